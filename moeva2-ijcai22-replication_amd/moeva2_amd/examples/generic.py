"""The two shipped constraint programs written as generic expressions.

``lcld_expressions()`` and ``botnet_expressions(feat_idx)`` restate, with the builder of
``moeva2_amd.attacks.moeva2.expr``, the columns of ``lcld_program`` and ``botnet_program``
(the dedicated ops of ``include/moeva_mi355x.h``): the same operands in the same order, so
on the device every generic column equals its dedicated op bit for bit.  They show how a new
dataset's constraints are written (``ExprConstraints``), and they are the input of the
generic-path tests and of ``tools/expr_speed.py``.

``lcld_tensor_expressions()`` and ``botnet_tensor_expressions(feat_idx)`` do the same for the
tensor paths (``lcld_tensor_program`` / ``botnet_tensor_program``, the reference's
``evaluate_tf2``), which C-PGD differentiates.  A tensor path is the smoothed form of the
numpy one: a guarded ratio ``where(b != 0, a / b, 0)`` has a NaN derivative for ``a`` at
``b = 0`` (the unselected branch still receives a zero adjoint, and 0 / 0 is NaN, in TF as
here), so the reference writes ``a / (b + alpha)`` there; and ``minimum(a, b)`` gives the
whole gradient to the smaller argument, the first on a tie.
"""
from ..attacks.moeva2.expr import (X, absolute, floor, isnan, maximum, minimum, mod, power,
                                   sum_of, where)
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


def lcld_tensor_expressions(alpha: float = 1e-5):
    """The 10 LCLD tensor-path columns (lcld_tensor_program; lcld_constraints.py:75-157)."""
    def installment(term):  # x0 r q / (q - 1), q = (1 + r)^term, r = x2 / 1200
        growth = power(1 + X[2] / 1200, term)
        return ((X[0] * (X[2] / 1200)) * growth) / (growth - 1)

    return [
        # TF_INSTALL_MIN: the nearer of the 36 and 60 month installments
        minimum(absolute(X[3] - installment(36)), absolute(X[3] - installment(60))) - 0.099999,
        maximum(alpha + X[10] - X[14], 0),                          # TF_HINGE_DIFF
        maximum(alpha + X[16] - X[11], 0),                          # TF_HINGE_DIFF
        minimum(absolute(36 - X[1]), absolute(60 - X[1])),          # TF_TERM_MIN
        _abs_ratio(20, 0, 6),
        _abs_ratio(21, 10, 14),
        absolute(X[22] - (_month(X[7]) - _month(X[9]))),            # MONTHDIFF
        _abs_ratio(23, 11, 22),
        _abs_ratio(24, 16, 22),
        # TF_RATIO_ALPHA_NEG: alpha in the denominator, -1 only where the plain ratio is NaN
        absolute(X[25] - where(isnan(X[16] / X[11]), -1, X[16] / (X[11] + alpha))),
    ]


def botnet_tensor_expressions(feat_idx: dict, alpha: float = 1e-5):
    """The 360 botnet tensor-path columns (botnet_tensor_program; botnet_constraints.py:48-115)."""
    fi = feat_idx
    out = []
    for d, off in (("s", 0.4999999), ("d", 0.0)):
        first = fi[f"icmp_sum_{d}_idx"] + fi[f"udp_sum_{d}_idx"] + fi[f"tcp_sum_{d}_idx"]
        second = fi[f"bytes_in_sum_{d}_idx"] + fi[f"bytes_out_sum_{d}_idx"]
        e = absolute(sum_of(first) - sum_of(second))
        out.append(e - off if off else e)  # TF_ABS_SUMDIFF_OFF / ABS_SUMDIFF
    for bo, po in (("bytes_out_sum_s_idx", "pkts_out_sum_s_idx"),
                   ("bytes_out_sum_d_idx", "pkts_out_sum_d_idx")):
        for j in range(len(bo) - 2):  # TF_RATIO_ALPHA_ZERO: isnan(a - b) ? 0 : a / (b + alpha)
            a, b = X[fi[bo][j]], X[fi[po][j]]
            out.append(where(isnan(a - b), 0, a / (b + alpha)))
    keys = list(fi.keys())
    for upper, lower in ((SUM_IDX, MAX_IDX), (SUM_IDX, MIN_IDX), (MAX_IDX, MIN_IDX)):
        for i in range(len(upper)):
            up_k, lo_k = keys[upper[i]], keys[lower[i]]
            for j in range(len(fi[up_k])):
                out.append(X[fi[lo_k][j]] - X[fi[up_k][j]])  # DIFF
    return out
