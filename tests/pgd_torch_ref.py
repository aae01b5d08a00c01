"""Torch CPU restatement of the C-PGD specification, shared by
tests/test_pgd_cpu.py and tests/test_gpu_pgd.py.  Not a conftest: imported by name.

It restates, with autograd and in fp32 or fp64: the tensor-path constraints of the LCLD and
botnet classes (the reference's evaluate_tf2), the Dense MLP, the two losses and one PGD
iteration.  Kink conventions are TF's: abs'(0) = 0, relu'(0) = 0, floor' = 0, floormod' = 1,
minimum gives the whole gradient to the smaller argument (the first on a tie), and the final
clamp passes gradient only where c - tol > 0.
"""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moeva2-ijcai22-replication_amd")
RES = os.path.join(PKG, "resources")
TOL, ALPHA = 1e-3, 1e-5
SUM_IDX = [0, 3, 6, 12, 15, 18]
MAX_IDX = [1, 4, 7, 13, 16, 19]
MIN_IDX = [2, 5, 8, 14, 17, 20]


def tmin(a, b):
    """tf.minimum with the gradient to the smaller argument, the first on a tie."""
    return torch.where(b < a, b, a)


def installment(x0, r, t):
    q = torch.pow(1 + r, t)
    return x0 * r * q / (q - 1)


def month(f):
    return torch.floor(f / 100) * 12 + torch.remainder(f, 100)


def lcld_tf(x):
    """lcld_constraints.py:75-157 (evaluate_tf2)."""
    r = x[:, 2] / 1200
    g41 = tmin(torch.abs(x[:, 3] - installment(x[:, 0], r, 36.0)),
               torch.abs(x[:, 3] - installment(x[:, 0], r, 60.0))) - 0.099999
    g42 = torch.relu(ALPHA + x[:, 10] - x[:, 14])
    g43 = torch.relu(ALPHA + x[:, 16] - x[:, 11])
    g44 = tmin(torch.abs(36 - x[:, 1]), torch.abs(60 - x[:, 1]))
    g45 = torch.abs(x[:, 20] - x[:, 0] / x[:, 6])
    g46 = torch.abs(x[:, 21] - x[:, 10] / x[:, 14])
    g47 = torch.abs(x[:, 22] - (month(x[:, 7]) - month(x[:, 9])))
    g48 = torch.abs(x[:, 23] - x[:, 11] / x[:, 22])
    g49 = torch.abs(x[:, 24] - x[:, 16] / x[:, 22])
    broken = x[:, 16] / x[:, 11]
    ratio = x[:, 16] / (x[:, 11] + ALPHA)
    g410 = torch.abs(x[:, 25] - torch.where(torch.isnan(broken), -torch.ones_like(ratio), ratio))
    c = torch.stack([g41, g42, g43, g44, g45, g46, g47, g48, g49, g410], 1)
    return torch.relu(c - TOL)


def load_feat_idx():
    with open(os.path.join(RES, "data", "botnet", "feat_idx.json")) as f:
        return json.load(f)


def botnet_tf(x, fi):
    """botnet_constraints.py:48-115, 235-269 (evaluate_tf2)."""
    def s(key):
        return x[:, fi[key]].sum(1)

    cols = []
    for d, off in (("s", 0.4999999), ("d", 0.0)):
        cols.append(torch.abs((s(f"icmp_sum_{d}_idx") + s(f"udp_sum_{d}_idx")
                               + s(f"tcp_sum_{d}_idx"))
                              - (s(f"bytes_in_sum_{d}_idx") + s(f"bytes_out_sum_{d}_idx"))) - off)
    for bo, po in (("bytes_out_sum_s_idx", "pkts_out_sum_s_idx"),
                   ("bytes_out_sum_d_idx", "pkts_out_sum_d_idx")):
        for j in range(len(bo) - 2):
            a, b = x[:, fi[bo][j]], x[:, fi[po][j]]
            ratio = a / (b + ALPHA)
            cols.append(torch.where(torch.isnan(a - b), torch.zeros_like(ratio), ratio))
    keys = list(fi.keys())
    for upper, lower in ((SUM_IDX, MAX_IDX), (SUM_IDX, MIN_IDX), (MAX_IDX, MIN_IDX)):
        for i in range(len(upper)):
            for j in range(len(fi[keys[upper[i]]])):
                cols.append(x[:, fi[keys[lower[i]]][j]] - x[:, fi[keys[upper[i]]][j]])
    return torch.relu(torch.stack(cols, 1) - TOL)


class Spec:
    """One project's attack in torch: weights, scaler, mask, constraint function."""

    def __init__(self, project, dtype=torch.float32, weights=None, biases=None):
        """weights / biases: an explicit Dense MLP (fp32 arrays, relu ... softmax) in place
        of the shipped nn.npz."""
        self.project, self.dtype = project, dtype
        if weights is None:
            d = np.load(os.path.join(RES, "models", project, "nn.npz"), allow_pickle=False)
            n = sum(1 for k in d.files if k.startswith("W"))
            weights = [d[f"W{i}"] for i in range(n)]
            biases = [d[f"b{i}"] for i in range(n)]
        # weights and scaler are fp32 values (what the device holds), widened for fp64
        self.W = [torch.tensor(np.asarray(w).astype(np.float32)).to(dtype) for w in weights]
        self.b = [torch.tensor(np.asarray(b).astype(np.float32)).to(dtype) for b in biases]
        sc = np.load(os.path.join(RES, "models", project, "scaler.npz"), allow_pickle=False)
        self.scale = torch.tensor(sc["scale_"].astype(np.float32)).to(dtype)
        self.min = torch.tensor(sc["min_"].astype(np.float32)).to(dtype)
        self.fi = load_feat_idx() if project == "botnet" else None

    def constraints(self, xf):
        return lcld_tf(xf) if self.project == "lcld" else botnet_tf(xf, self.fi)

    def unscale(self, x):
        return (x - self.min) / self.scale

    def rescale(self, xf):
        return xf * self.scale + self.min

    def logits(self, x):
        h = x
        for W, b in zip(self.W[:-1], self.b[:-1]):
            h = torch.relu(h @ W + b)
        return h @ self.W[-1] + self.b[-1]

    def predict(self, x):
        return torch.argmax(self.logits(torch.as_tensor(x, dtype=self.dtype)), 1)

    def grad(self, x, y, mode):
        """(gradient, loss_class, constraint sum, columns) of classifier.py:107-332."""
        x = torch.as_tensor(x, dtype=self.dtype).clone().requires_grad_(True)
        y = torch.as_tensor(y, dtype=torch.long)
        loss_class = torch.nn.functional.cross_entropy(self.logits(x), y, reduction="none")
        cols = self.constraints(self.unscale(x))
        csum = cols.sum(1)
        if "constraints+flip" in mode:
            loss = loss_class - csum
        elif "constraints" in mode:
            loss = -csum
        else:
            loss = loss_class
        (g,) = torch.autograd.grad(loss.sum(), x)
        return g.detach(), loss_class.detach(), csum.detach(), cols.detach()

    def repair(self, xf, ohe_groups):
        """lcld_constraints.py:40-66 on feature-space rows."""
        if self.project != "lcld":
            return xf
        xf = xf.clone()
        x1 = torch.where(xf[:, 1] < 48, torch.full_like(xf[:, 1], 36.0),
                         torch.full_like(xf[:, 1], 60.0))
        xf[:, 1] = x1
        xf[:, 3] = installment(xf[:, 0], xf[:, 2] / 1200, x1)
        for m in ohe_groups:
            m = torch.as_tensor(np.asarray(m), dtype=torch.long)
            am = torch.argmax(xf[:, m], 1)
            xf[:, m] = torch.nn.functional.one_hot(am, len(m)).to(xf.dtype)
        return xf

    def step(self, x, x_init, g, mask, norm, eps, eta, repair=False, ohe_groups=()):
        """atk.py:74-163 steps 2-8 in this object's dtype; g is the raw gradient."""
        dt = self.dtype
        x, x_init, g = (torch.as_tensor(v, dtype=dt) for v in (x, x_init, g))
        eps, eta, tiny = (torch.tensor(v, dtype=dt) for v in (eps, eta, 1e-7))
        g = torch.where(torch.isnan(g), torch.zeros_like(g), g)
        g = torch.where(torch.as_tensor(mask).bool(), g, torch.zeros_like(g))
        if norm == 2:
            g = g / (torch.sqrt((g * g).sum(1, keepdim=True)) + tiny)
        else:
            g = torch.sign(g)
        x = torch.clamp(x + eta * g, 0, 1)
        d = x - x_init
        if norm == 2:
            d = d * torch.minimum(torch.ones((), dtype=dt),
                                  eps / (torch.sqrt((d * d).sum(1, keepdim=True)) + tiny))
        else:
            d = torch.sign(d) * torch.minimum(torch.abs(d), eps)
        x = x_init + d
        if repair:
            x = self.rescale(self.repair(self.unscale(x), ohe_groups))
        return x

    def attack(self, x_init, mask, mode, norm, eps, max_iter, eps_step=0.1, ohe_groups=(),
               y=None):
        """y: labels (n,); None: the model's own prediction on x_init."""
        x_init = torch.as_tensor(x_init, dtype=self.dtype)
        y = self.predict(x_init) if y is None else torch.as_tensor(np.asarray(y), dtype=torch.long)
        x = x_init.clone()
        for i in range(max_iter):
            g = self.grad(x, y, mode)[0]
            eta = eps_step
            if "adaptive_eps_step" in mode:
                eta = float(eps * (1 / np.float_power(10.0, np.float64(i // (max_iter // 7) + 1))))
            x = self.step(x, x_init, g, mask, norm, eps, eta, "repair" in mode, ohe_groups)
        return x


def _row_sum_device_order(v):
    """Sum over a row's features in the kernel's order (csrc/pgd.hip pgd_step): four fp32
    partial sums over features p, p + 4, ... taken sequentially, then (s0 + s1) + (s2 + s3)."""
    v = np.asarray(v, np.float32)
    parts = []
    for p in range(4):
        cs = np.cumsum(v[:, p::4], axis=1, dtype=np.float32)
        parts.append(cs[:, -1] if cs.shape[1] else np.zeros(v.shape[0], np.float32))
    return ((parts[0] + parts[1]) + (parts[2] + parts[3]))[:, None]


def step_device_order(x, x_init, g, mask, norm, eps, eta):
    """Steps 2-7 of the attack loop in numpy fp32 with the kernel's summation order (every
    other operation is a single correctly rounded fp32 operation on both sides)."""
    f = np.float32
    x, x_init, g = (np.asarray(v, f) for v in (x, x_init, g))
    eps, eta = f(eps), f(eta)
    g = np.where(np.isnan(g), f(0), g)
    g = np.where(np.asarray(mask).astype(bool), g, f(0)).astype(f)
    if norm == 2:
        g = g / (np.sqrt(_row_sum_device_order(g * g)) + f(1e-7))
    else:
        g = np.sign(g)
    x = np.clip(x + eta * g, f(0), f(1))
    d = x - x_init
    if norm == 2:
        q = eps / (np.sqrt(_row_sum_device_order(d * d)) + f(1e-7))
        d = d * np.where(q < 1, q, f(1)).astype(f)
    else:
        d = np.sign(d) * np.minimum(np.abs(d), eps)
    return (x_init + d).astype(f)


def numpy_program(code, arg, karg, pool, x, OP, tol=TOL):
    """Numpy statement of the tensor-path ops (include/moeva_mi355x.h MV_OP_*), fp64."""
    x = np.asarray(x, np.float64)
    inv = {v: k for k, v in OP.items()}
    cols = []
    with np.errstate(all="ignore"):
        for j in range(len(code)):
            a, k0, op = arg[j], karg[j][0], inv[int(code[j])]
            X = lambda i: x[:, a[i]]  # noqa: E731
            if op == "DIFF":
                c = X(0) - X(1)
            elif op in ("ABS_SUMDIFF", "TF_ABS_SUMDIFF_OFF"):
                c = np.abs(x[:, pool[a[0]:a[1]]].sum(1) - x[:, pool[a[1]:a[2]]].sum(1)) - k0
            elif op == "TF_INSTALL_MIN":
                r = X(2) / 1200

                def inst(t):
                    q = np.power(1 + r, t)
                    return X(0) * r * q / (q - 1)

                c = np.minimum(np.abs(X(3) - inst(36)), np.abs(X(3) - inst(60))) - k0
            elif op == "TF_HINGE_DIFF":
                c = np.maximum(k0 + X(0) - X(1), 0)
            elif op == "TF_TERM_MIN":
                c = np.minimum(np.abs(36 - X(0)), np.abs(60 - X(0)))
            elif op == "ABS_RATIO":
                c = np.abs(X(0) - X(1) / X(2))
            elif op == "MONTHDIFF":
                m = lambda f: np.floor(f / 100) * 12 + np.mod(f, 100)  # noqa: E731
                c = np.abs(X(0) - (m(X(1)) - m(X(2))))
            elif op == "TF_RATIO_ALPHA_NEG":
                c = np.abs(X(0) - np.where(np.isnan(X(1) / X(2)), -1.0, X(1) / (X(2) + k0)))
            elif op == "TF_RATIO_ALPHA_ZERO":
                c = np.where(np.isnan(X(0) - X(1)), 0.0, X(0) / (X(1) + k0))
            else:
                raise ValueError(op)
            cols.append(c)
    return np.maximum(np.column_stack(cols) - tol, 0)
