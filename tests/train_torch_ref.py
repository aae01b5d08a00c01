"""Torch CPU restatement of the training step, shared by
tests/test_train_cpu.py and tests/test_gpu_train.py.  Not a conftest: imported by name.

The same loop as mv_train_steps in fp32 or fp64: explicit permutation, batch slicing (a short
last batch divides by its own size), mean cross-entropy from the logits, autograd, and
Keras-form Adam

    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  w -= lr_t m / (sqrt(v) + eps),
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)   (fp64 on the host, then the helper's dtype).

Weights are read as fp32 values (pgd_torch_ref.Spec) and widened for fp64.  The flat
parameter layout is the device's: per layer W row-major (in, out), then b.
"""
import numpy as np
import torch

import pgd_torch_ref as ref

ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7)


def flatten(W, b):
    return np.concatenate([np.concatenate([np.asarray(w).ravel(), np.asarray(v).ravel()])
                           for w, v in zip(W, b)])


def layer_slices(dims):
    """Per layer, the slice of the flat layout holding its W and b."""
    out, o = [], 0
    for k, n in zip(dims[:-1], dims[1:]):
        out.append(slice(o, o + k * n + n))
        o += k * n + n
    return out


class TrainRef:
    """One model being trained, in ``dtype``."""

    def __init__(self, weights, biases, dtype=torch.float32, **adam):
        self.dtype = dtype
        # fp32 values, widened (pgd_torch_ref.Spec's rule)
        self.W = [torch.tensor(np.asarray(w).astype(np.float32)).to(dtype) for w in weights]
        self.b = [torch.tensor(np.asarray(v).astype(np.float32)).to(dtype) for v in biases]
        self.m = [torch.zeros_like(p) for p in self.params()]
        self.v = [torch.zeros_like(p) for p in self.params()]
        self.t = 0
        self.opt = dict(ADAM, **adam)

    @classmethod
    def shipped(cls, project, dtype=torch.float32, **adam):
        s = ref.Spec(project, dtype)
        return cls([w.numpy() for w in s.W], [v.numpy() for v in s.b], dtype, **adam)

    def params(self):
        """W0, b0, W1, b1, ...: the flat layout's order."""
        return [p for pair in zip(self.W, self.b) for p in pair]

    def dims(self):
        return [self.W[0].shape[0]] + [w.shape[1] for w in self.W]

    def logits(self, x):
        h = torch.as_tensor(x, dtype=self.dtype)
        for W, b in zip(self.W[:-1], self.b[:-1]):
            h = torch.relu(h @ W + b)
        return h @ self.W[-1] + self.b[-1]

    def loss(self, x, y):
        y = torch.as_tensor(np.asarray(y), dtype=torch.long)
        return torch.nn.functional.cross_entropy(self.logits(x), y, reduction="mean")

    def grad(self, x, y):
        """(flat gradient, loss) of the mean cross-entropy over the rows, numpy."""
        ps = self.params()
        for p in ps:
            p.requires_grad_(True)
        loss = self.loss(x, y)
        gs = torch.autograd.grad(loss, ps)
        for p in ps:
            p.requires_grad_(False)
        return np.concatenate([g.numpy().ravel() for g in gs]), float(loss.detach())

    def step(self, x, y):
        """One Adam step on the batch; returns its loss (before the update)."""
        g, loss = self.grad(x, y)
        self.t += 1
        o, dt = self.opt, self.dtype
        lr_t = o["lr"] * np.sqrt(1.0 - o["beta2"] ** self.t) / (1.0 - o["beta1"] ** self.t)
        lr_t, b1, b2, eps = (torch.tensor(v, dtype=dt)
                             for v in (lr_t, o["beta1"], o["beta2"], o["epsilon"]))
        off = 0
        with torch.no_grad():
            for p, m, v in zip(self.params(), self.m, self.v):
                gp = torch.as_tensor(g[off:off + p.numel()], dtype=dt).reshape(p.shape)
                off += p.numel()
                m.copy_(b1 * m + (1 - b1) * gp)
                v.copy_(b2 * v + (1 - b2) * (gp * gp))
                p.sub_((lr_t * m) / (torch.sqrt(v) + eps))
        return loss

    def steps(self, x, y, batch, n_steps, first_row=0, perm=None):
        """mv_train_steps: step s takes positions first_row + s batch ... of the permuted
        order, at most batch and none past n.  Returns the steps' losses."""
        x, y = np.asarray(x), np.asarray(y)
        n = x.shape[0]
        order = np.arange(n) if perm is None else np.asarray(perm)
        losses = []
        for s in range(n_steps):
            rows = order[first_row + s * batch: min(n, first_row + (s + 1) * batch)]
            assert rows.size > 0
            losses.append(self.step(x[rows], y[rows]))
        return np.array(losses)

    def eval(self, x, y):
        """(mean cross-entropy, argmax-correct count, per-row logit margin between the two
        largest logits)."""
        z = self.logits(x)
        yt = torch.as_tensor(np.asarray(y), dtype=torch.long)
        loss = float(torch.nn.functional.cross_entropy(z, yt, reduction="mean"))
        correct = int((torch.argmax(z, 1) == yt).sum())
        if z.shape[1] > 1:
            top = torch.topk(z, 2, dim=1).values
            margin = (top[:, 0] - top[:, 1]).numpy()
        else:
            margin = np.full(z.shape[0], np.inf)
        return loss, correct, margin

    def flat(self):
        return flatten([w.numpy() for w in self.W], [v.numpy() for v in self.b])

    def flat_state(self):
        return (np.concatenate([m.numpy().ravel() for m in self.m]),
                np.concatenate([v.numpy().ravel() for v in self.v]))


def numpy_backward(W, b, x, y):
    """Hand-written fp64 backward of the mean cross-entropy (the self-check's oracle): flat
    gradient in the device layout."""
    W = [np.asarray(w, np.float64) for w in W]
    b = [np.asarray(v, np.float64) for v in b]
    x, y = np.asarray(x, np.float64), np.asarray(y)
    acts = [x]
    for w, v in zip(W[:-1], b[:-1]):
        acts.append(np.maximum(acts[-1] @ w + v, 0.0))
    z = acts[-1] @ W[-1] + b[-1]
    z = z - z.max(1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    dz = p.copy()
    dz[np.arange(len(y)), y] -= 1.0
    dz /= len(y)
    gW, gb = [None] * len(W), [None] * len(W)
    for l in range(len(W) - 1, -1, -1):
        gW[l] = acts[l].T @ dz
        gb[l] = dz.sum(0)
        if l > 0:
            dz = (dz @ W[l].T) * (acts[l] > 0)
    return flatten(gW, gb)


def adam_numpy_fp32(w, m, v, g, t, lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7):
    """k_train_adam's arithmetic in numpy fp32, operation for operation: every step is one
    correctly rounded fp32 operation on both sides.  Returns (w, m, v)."""
    f = np.float32
    w, m, v, g = (np.asarray(a, f) for a in (w, m, v, g))
    lr_t = f(lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
    b1, b2, eps = f(beta1), f(beta2), f(epsilon)
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * (g * g)
    w = w - (lr_t * m) / (np.sqrt(v) + eps)
    return w.astype(f), m.astype(f), v.astype(f)


def blobs(n=2048, d=47, seed=0):
    """Two Gaussian blobs, means 0.5 -+ 0.15, sigma 0.1, clipped to [0, 1]; labels 0 / 1."""
    rng = np.random.default_rng(seed)
    y = (np.arange(n) % 2).astype(np.int32)
    x = 0.5 + np.where(y[:, None] == 1, 0.15, -0.15) + 0.1 * rng.standard_normal((n, d))
    return np.clip(x, 0, 1).astype(np.float32), y
