"""oracle/device_order.py's restatement of k_mlpw32 (the fp32 wide classifier), checked on the
CPU before any GPU test leans on it: it is the same function as the fp32 numpy forward up to
fp32 rounding, and with the last Dense layer confined to column tile 0 it equals a sum written
out by hand here (one product per lane, the 16-lane butterfly, nothing from the other waves),
so an indexing slip in the restatement cannot hide behind the kernel it restates."""
import dataclasses

import numpy as np
import pytest

from oracle import device_order as do
from oracle import moeva_oracle as mo
from oracle.problems import Project


def _net(dims, seed):
    rng = np.random.default_rng(seed)
    W = [(rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32)
         for a, b in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * rng.standard_normal(b)).astype(np.float32) for b in dims[1:]]
    return W, bs


@pytest.fixture(scope="module")
def lcld():
    p = Project("lcld")
    rng = np.random.default_rng(2)
    prob = p.problem(p.x[0])
    gl, gu = mo.genetic_bounds(p.lay, prob.xl, prob.xu)
    isr = np.array([t == "real" for t in mo.genetic_types(p.lay)])
    g = np.repeat(mo.initial_population(prob, 1), 21, axis=0)
    for r in range(g.shape[0]):
        k = rng.integers(0, p.lay.V, size=1 + r % 5)
        v = rng.uniform(gl[k], gu[k])
        g[r, k] = np.where(isr[k], v, np.round(v))
    return p, prob, mo.genetic_to_ml(p.lay, g, prob.x_init)


def _fma(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


@pytest.mark.parametrize("dims", [(47, 144, 272, 3), (47, 400, 2)])
def test_mlpw32_order_is_the_fp32_forward(lcld, dims):
    p, prob, x_f = lcld
    W, bs = _net(dims, 5)
    assert do.mlpw32_cj(dataclasses.replace(prob, weights=W, biases=bs)) == 4
    ref = mo.mlp_predict_proba(x_f * p.ml[0] + p.ml[1], W, bs)
    for mc in range(dims[-1]):
        pr = dataclasses.replace(prob, weights=W, biases=bs, minimize_class=mc)
        got = do.f1_device_order(pr, x_f, kernel="mlpw32")
        np.testing.assert_allclose(got, ref[:, mc], rtol=1e-5, atol=1e-7)
        # k_mlp2's order is another rounding of the same sum
        np.testing.assert_allclose(do.f1_device_order(pr, x_f), ref[:, mc], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("dims", [(47, 144, 272, 3), (47, 400, 2)])
def test_mlpw32_order_single_tile_by_hand(lcld, dims):
    p, prob, x_f = lcld
    W, bs = _net(dims, 6)
    W[-1][16:] = 0  # only column tile 0 of the last hidden layer (wave 0, j = 0) contributes
    pr = dataclasses.replace(prob, weights=W, biases=bs, minimize_class=dims[-1] - 1)
    got = do.f1_device_order(pr, x_f, kernel="mlpw32")
    # hidden layers, scalar by scalar: layer 0 over the mutable features (zero padded to a
    # multiple of 16) plus the immutable features' fmaf chain in the bias
    mut = np.where(p.lay.mutable_mask)[0]
    imm = np.where(~np.asarray(p.lay.mutable_mask, bool))[0]
    x32 = (x_f * p.ml[0] + p.ml[1]).astype(np.float32)
    x0 = (prob.x_init * p.ml[0] + p.ml[1]).astype(np.float32)
    n_cls = dims[-1]
    x_f = x_f[:6]  # rows with 1..5 and 1 perturbed genes: the scalar loops are slow
    got = got[:6]
    want = np.empty(x_f.shape[0])
    for r in range(x_f.shape[0]):
        h = np.zeros(-(-mut.size // 16) * 16, np.float32)
        h[:mut.size] = x32[r, mut]
        for l in range(len(W) - 1):
            Wl = W[l]
            if l == 0:
                Wl = np.zeros((h.size, W[0].shape[1]), np.float32)
                Wl[:mut.size] = W[0][mut]
            # the zeroed last layer reads columns 0..15 of the last hidden layer only
            out = np.zeros(Wl.shape[1], np.float32)
            for col in (range(Wl.shape[1]) if l + 2 < len(W) else range(16)):
                acc = np.float32(0)
                for kg in range(h.size // 16):
                    for s in range(4):
                        for ka in range(4):
                            k = 16 * kg + 4 * ka + s
                            acc = _fma(h[k], Wl[k, col], acc)
                b = bs[l][col]
                if l == 0:
                    t = np.float32(0)
                    for f in imm:
                        t = _fma(x0[f], W[0][f, col], t)
                    b = np.float32(b + t)
                out[col] = max(np.float32(acc + b), np.float32(0))
            h = out
        z = np.empty(n_cls, np.float32)
        for c in range(n_cls):
            v = [np.float32(h[il] * W[-1][il, c]) for il in range(16)]
            while len(v) > 1:
                v = [np.float32(v[2 * i] + v[2 * i + 1]) for i in range(len(v) // 2)]
            z[c] = np.float32(v[0] + bs[-1][c])
        want[r] = do.softmax_keras32(z[None, :])[0, n_cls - 1]
    np.testing.assert_array_equal(got, want)
