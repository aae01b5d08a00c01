"""The engine's bf16 perf-mode classifier (mv_set_mlp_precision) restated in numpy (helper
module, not a test file; test infrastructure, not an oracle of the reference).

Every variant computes the same arithmetic: layer 0 over the mutable features ``mut`` with the
other features folded into an fp32 per-row bias as k_setup_states folds them (``bias1``: an
fp32 fmaf chain over those features in ascending order from 0.f, then b1 + s in fp32 -- the
chain oracle/device_order.layer0_bias restates and every fp32 route test holds bit for bit;
folded in fp64 it lies up to a few fp32 ulps of a hidden activation away, which is enough to
carry an activation over a bf16 tie), the MFMA layers' weights and activations rounded to
bf16 to nearest even, exact products, fp32 biases, ReLU, and the last Dense + softmax in fp32
from the fp32 activations of the last hidden layer.  They differ in how a layer's products
are accumulated:

  A  in fp64, rounded to fp32 once per layer;
  B  an fp32 accumulator advanced once per step of 32 k, steps ascending: a step's 32 products
     are summed in fp64 (exact to 2^-53: the v_mfma_f32_16x16x32_bf16 order inside a step is
     not documented) and added with one rounding;
  C  as B with the steps descending.

The accumulated fp32 error moves hidden activations across bf16 rounding boundaries; a moved
activation changes f1 by far more than fp32 rounding.  That is the device's legitimate slack,
and the spread of A, B and C on a case's own rows measures it: ``floor`` (DESIGN.md section 7a's
rule: the reference's own spread, the device is allowed 4 x)."""
import numpy as np

from oracle import device_order as do


def bf16(a):
    """fp32 -> bf16 -> fp32, round to nearest even (v_cvt_pk_bf16_f32 on finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _layer(h, w, bias, variant):
    """relu(bf16(h) . bf16(w) + bias) as fp32; bias fp64 (n, N) or fp32 (N,)."""
    a, b = bf16(h).astype(np.float64), bf16(w).astype(np.float64)
    if variant == "A":
        return np.maximum((a @ b + bias).astype(np.float32), 0)
    K = a.shape[1]
    steps = list(range(0, K, 32))
    if variant == "C":
        steps.reverse()
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in steps:
        acc = (acc.astype(np.float64) + a[:, k:k + 32] @ b[k:k + 32]).astype(np.float32)
    return np.maximum((acc.astype(np.float64) + bias).astype(np.float32), 0)


def bias1_fold(x, imm, W0, b1):
    """k_setup_states: b1 + the fmaf chain over the features ``imm`` (ascending) of the fp32
    rows x, every step rounded to fp32 (a * b exact in fp64, one rounding of the sum)."""
    s = np.zeros((x.shape[0], W0.shape[1]), np.float32)
    for f in imm:
        s = (x[:, f:f + 1].astype(np.float64) * W0[f][None, :].astype(np.float64)
             + s.astype(np.float64)).astype(np.float32)
    return (b1.astype(np.float32) + s).astype(np.float32)


def bf16_forward(x_ml, mut, W, bs, variant="A"):
    """(n, D) ML-scaled rows -> (n, classes) probabilities.  ``mut``: the features layer 0
    multiplies in bf16 (the engine's mutable features; for an attack on the compact gene
    layout, the stored ones: the fixed ones join the fp32 bias fold)."""
    if variant not in ("A", "B", "C"):
        raise ValueError(variant)
    x = np.asarray(x_ml, np.float64).astype(np.float32)
    imm = np.setdiff1d(np.arange(x.shape[1]), mut)
    h = _layer(x[:, mut], W[0][mut], bias1_fold(x, imm, W[0], bs[0]), variant)
    for w, b in zip(W[1:-1], bs[1:-1]):
        h = _layer(h, w, b, variant)
    # the last Dense and the softmax in fp32: an fmaf chain over k from 0.f, + b, Keras's fp32
    # softmax (the kernels split the chain differently; fp32 rounding either way)
    Wl = W[-1].astype(np.float32)
    z = do._dense_seq(h, Wl, Wl.shape[0]) + bs[-1].astype(np.float32)
    return do.softmax_keras32(z).astype(np.float64)


FLOOR_MIN = 2.0 ** -20


def f1_with_floor(x_ml, mut, W, bs, cls):
    """(variant A's f1 of class ``cls``, floor): floor = the largest pairwise |f1| difference
    among A, B and C on these rows, at least 2^-20."""
    f = [bf16_forward(x_ml, mut, W, bs, v)[:, cls] for v in "ABC"]
    spread = max(float(np.abs(f[i] - f[j]).max()) for i, j in ((0, 1), (0, 2), (1, 2)))
    return f[0], max(spread, FLOOR_MIN)
