"""Every product route of the Dense-ReLU classifier (launch_mlp / launch_predict in
csrc/eval.hip), each pinned on nets with random NON-ZERO biases in every layer, more than two
classes, and the widths at which a kernel's guards change side:

  * k_mlpw32 (fp32, hidden widths above 128): its three column-tiles-per-wave instances, a
    wave left without a column tile, an odd number of 16-k groups, one hidden layer, and the
    LCLD route (fp32 rows from k_narrow) -- bit-identical to oracle/device_order's
    ``kernel="mlpw32"`` restatement;
  * k_mlp2 in fp32 at hidden widths 65..128, reading the genes (botnet) and the fp32 ML rows
    (LCLD), and k_mlpr on ML rows with more than two classes -- bit-identical to
    f1_device_order;
  * k_predict at the 16- / 32-row tile edges against an fp64 forward of the same weights;
  * k_mlpw (bf16) at its two- and four-tile instances with biases, against the numpy
    restatement of the bf16 arithmetic.

Each test asserts the kernel kind the engine reports, so a routing change cannot move a test
onto another kernel unnoticed.  The k_mlp fallback (32-row tiles) has its own files:
tests/test_gpu_mlp_fallback.py (fp32, bit for bit) and tests/test_gpu_bf16_routes.py (every
bf16 instance, k_mlp<4|8,true> among them).  In the product it takes the wide nets whose
64-row tile passes the CU's 160 KiB (tests/test_routes_cpu.py pins the selection and the
edges): fp32 with k_mlpw32's tile from Dm4 624 (a 512-512-2 net) or 640 (512-256-2) on, bf16
with k_mlpw's from about Dm4 608 on, or on botnet (Dm4 432) with a 512-wide last hidden layer
and 8 classes.  Hidden widths that are no multiple of 16 or above 512 and nets of more than 8
classes never reach a kernel: mv_engine_create refuses them, as it refuses a problem whose
k_mlp tile itself passes 160 KiB (a 512-512-2 net from Dm4 736 on)."""
import dataclasses

import numpy as np
import pytest

from oracle import moeva_oracle as mo
from oracle.problems import Project
import bf16_ref
from test_gpu_parity import make_constraints, make_scaler

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _net(dims, seed):
    """Dense relu .. softmax, weights ~ N(0, 1/fan_in), every bias 0.1 * N(0, 1)."""
    rng = np.random.default_rng(seed)
    W = [(rng.standard_normal((a, b)) / np.sqrt(a)).astype(np.float32)
         for a, b in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * rng.standard_normal(b)).astype(np.float32) for b in dims[1:]]
    return W, bs


def _classifier(W, bs):
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.io.tf_bundle import DenseMLP

    return Classifier(DenseMLPModel(DenseMLP(W, bs, ["relu"] * (len(W) - 1) + ["softmax"])))


def _forward64(x_ml, W, bs):
    """The plain reference: the fp32 weights and the fp32-cast input, every operation in fp64."""
    h = np.asarray(x_ml, np.float64).astype(np.float32).astype(np.float64)
    for i, (w, b) in enumerate(zip(W, bs)):
        h = h @ w.astype(np.float64) + b.astype(np.float64)
        if i + 1 < len(W):
            h = np.maximum(h, 0.0)
    e = np.exp(h - h.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


_PROJECTS = {}


def _project(name):
    if name not in _PROJECTS:
        p = Project(name)
        c = make_constraints(name)
        _PROJECTS[name] = (p, c, make_scaler(name))
    return _PROJECTS[name]


def _perturbed_genes(p, probs, n, rng):
    """n rows per state: the initial genes with 1..5 positions redrawn inside the bounds."""
    isr = np.array([t == "real" for t in mo.genetic_types(p.lay)])
    genes = np.empty((len(probs), n, p.lay.V))
    for b, prob in enumerate(probs):
        gl, gu = mo.genetic_bounds(p.lay, prob.xl, prob.xu)
        g = np.repeat(mo.initial_population(prob, 1), n, axis=0)
        for r in range(n):
            k = rng.integers(0, p.lay.V, size=1 + r % 5)
            v = rng.uniform(gl[k], gu[k])
            g[r, k] = np.where(isr[k], v, np.round(v))
        genes[b] = g
    return genes


def check_route(name, dims, kind, kernel, seed):
    """mv_evaluate's F on 3 states x 37 rows (111 rows: two 64-row tiles, the second partial,
    one spanning two states' bias1 rows), then a 4-generation attack's final F (the compact
    gene layout on botnet, offspring rows through out_map), both bit-identical to the oracle
    in the engine's order (``kernel``: device_order's classifier order).  LCLD's f3 keeps the
    1e-14 of test_evaluate_bit_exact_in_engine_order (device pow against numpy's)."""
    from oracle import device_order as do
    from moeva2_amd.attacks.moeva2.ref_dirs import energy_ref_dirs
    from moeva2_amd.problem import build_device_program, get_engine

    p, c, sc = _project(name)
    W, bs = _net(dims, seed)
    codes = build_device_program(c).op_code
    eng = get_engine(c, _classifier(W, bs), sc, 2)
    X = p.x[:3]
    bounds = [c.get_feature_min_max(dynamic_input=x) for x in X]
    eng.set_states(X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]), 1)
    assert eng.kernel_times()["mlp_kernel"] == kind
    probs = [dataclasses.replace(p.problem(X[b], minimize_class=1), weights=W, biases=bs)
             for b in range(3)]
    n = 37
    genes = _perturbed_genes(p, probs, n, np.random.default_rng(seed + 1))
    F = torch.empty((3, n, 3), dtype=torch.float64, device="cuda")
    eng.evaluate(torch.as_tensor(genes, device="cuda"), F)
    torch.cuda.synchronize()
    F = F.cpu().numpy()

    def compare(Fd, prob, g, fixed, what):
        x_ml = mo.genetic_to_ml(p.lay, g, prob.x_init) * p.ml[0] + p.ml[1]
        f64 = _forward64(x_ml, W, bs)[:, 1]
        err = float(np.abs(Fd[:, 0] - f64).max())
        # a kernel wrong in a bias row, a column tile or a class misses the fp64 forward by far
        # more than fp32 rounding: tell that apart from a slip in the restated ORDER below
        np.testing.assert_allclose(Fd[:, 0], f64, rtol=1e-5, atol=1e-7)
        ref = do.evaluate_device_order(prob, g, codes, fixed=fixed, kernel=kernel)
        np.testing.assert_array_equal(Fd[:, :2], ref[:, :2], err_msg=what)
        if name == "botnet":  # botnet constraints call no pow
            np.testing.assert_array_equal(Fd[:, 2], ref[:, 2], err_msg=what)
        else:
            np.testing.assert_allclose(Fd[:, 2], ref[:, 2], rtol=1e-14, atol=0, err_msg=what)
        return err

    worst = max(compare(F[b], probs[b], genes[b], None, f"evaluate, state {b}")
                for b in range(3))
    eng.attack_run(4, 23, 10, seed, energy_ref_dirs(3, 20, 1), 0.05, 0)
    ga = torch.empty((3, 23, p.lay.V), dtype=torch.float64, device="cuda")
    Fa = torch.empty((3, 23, 3), dtype=torch.float64, device="cuda")
    eng.attack_population(ga, Fa)
    torch.cuda.synchronize()
    stored = eng.stored_genes()
    fixed = None  # one-hot layouts (LCLD) are never compacted
    if name == "botnet":
        fixed = np.zeros(p.lay.mutable_mask.shape[0], bool)
        fixed[np.where(p.lay.mutable_mask)[0][~stored]] = True
    else:
        assert stored.all()
    ga, Fa = ga.cpu().numpy(), Fa.cpu().numpy()
    worst = max([worst] + [compare(Fa[b], probs[b], ga[b], fixed, f"attack, state {b}")
                           for b in range(3)])
    print(f"{kind} {name} {'-'.join(map(str, dims))}: max |f1 - fp64 forward| {worst:.3e}")


# ------------------------------------------------------------------ k_mlpw32
@pytest.mark.parametrize("name,dims", [
    ("botnet", (756, 144, 2)),            # one hidden layer; CJ 2; 9 tiles: wave 0 two, the rest one
    ("botnet", (756, 272, 144, 3)),       # CJ 4 with 17 tiles; K 272: 17 k-groups, the odd tail
    ("botnet", (756, 400, 512, 8)),       # 25 tiles: wave 0 four, the rest three; full 512
    ("botnet", (756, 256, 2)),            # exact fit, CJ 2
    ("botnet", (756, 512, 512, 256, 2)),  # exact fit, CJ 4 (BASELINE configs[4]'s shape)
    ("lcld", (47, 144, 272, 3)),          # fp32 rows from k_narrow, small Dm4
    ("lcld", (47, 512, 2))])
def test_wide_fp32_classifier_bit_exact(name, dims):
    check_route(name, dims, "k_mlpw32", "mlpw32", 21)


# ------------------------------------------------------------------ k_mlp2, fp32, CJ = 2
@pytest.mark.parametrize("name,dims,kind", [
    ("botnet", (756, 128, 2), "k_mlp2(genes)"),
    ("botnet", (756, 80, 128, 3), "k_mlp2(genes)"),
    ("botnet", (756, 32, 112, 48, 2), "k_mlp2(genes)"),  # a narrow layer under a CJ 2 instance
    ("lcld", (47, 96, 80, 2), "k_mlp2"),
    ("lcld", (47, 128, 5), "k_mlp2")])
def test_mlp2_fp32_two_column_tiles_bit_exact(name, dims, kind):
    check_route(name, dims, kind, "mlp2", 31)


# ------------------------------------------------------------------ k_mlpr on ML rows
@pytest.mark.parametrize("dims", [(47, 48, 32, 3), (47, 64, 8)])
def test_row_classifier_ml_rows_multiclass_bit_exact(dims):
    check_route("lcld", dims, "k_mlpr", "mlp2", 41)


# ------------------------------------------------------------------ k_predict
_PREDICT_NETS = [(47, 64, 32, 3), (47, 128, 8), (47, 256, 144, 2), (756, 48, 2),
                 (756, 512, 272, 3)]  # the last: the 16-row-tile instance
_PREDICT_ROWS = (1, 15, 16, 17, 31, 32, 33, 65)


@pytest.fixture(scope="module")
def predict_inputs():
    """65 ML-scaled candidate rows per project, rounded to fp32 (the classifier's input cast is
    then exact), with the fp64 forward of every net computed once."""
    out = {}
    for name, D in (("lcld", 47), ("botnet", 756)):
        p = _project(name)[0]
        x = (p.x[:65] * p.ml[0] + p.ml[1]).astype(np.float32).astype(np.float64)
        assert x.shape == (65, D)
        out[D] = x
    refs = {}
    for dims in _PREDICT_NETS:
        W, bs = _net(dims, 51)
        refs[dims] = (W, bs, _forward64(out[dims[0]], W, bs))
    return out, refs


@pytest.mark.parametrize("dims", _PREDICT_NETS, ids=lambda d: "-".join(map(str, d)))
def test_predict_proba_tile_edges(predict_inputs, dims):
    """Classifier.predict_proba at row counts on both sides of the 16- and 32-row tile edges and
    over several workgroups, 3 and 8 classes, non-zero biases: rows sum to 1 and match the fp64
    forward at the project's f1 tolerance.  The same rows again straight from a device buffer
    whose rows past n hold 1e6 and into an output buffer with sentinel rows past n: a kernel
    that reads or writes past n changes a probability or a sentinel."""
    from moeva2_amd import _native

    xs, refs = predict_inputs
    W, bs, ref = refs[dims]
    x = xs[dims[0]]
    # the fp32 numpy forward itself stays inside the tolerance on these rows, so the bound is
    # fp32 rounding's and not this net's luck
    np.testing.assert_allclose(mo.mlp_predict_proba(x, W, bs), ref, rtol=1e-5, atol=1e-7)
    clf = _classifier(W, bs)
    mlp = _native.Mlp(W, bs)
    worst = 0.0
    for n in _PREDICT_ROWS:
        got = clf.predict_proba(x[:n])
        assert got.shape == (n, dims[-1])
        np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-6)
        np.testing.assert_allclose(got, ref[:n], rtol=1e-5, atol=1e-7)
        worst = max(worst, float(np.abs(got - ref[:n]).max()))
        pad = -(-n // 32) * 32 + 32
        xd = torch.full((pad, dims[0]), 1e6, dtype=torch.float64, device="cuda")
        xd[:n] = torch.from_numpy(x[:n])
        od = torch.full((pad, dims[-1]), -7.0, dtype=torch.float64, device="cuda")
        mlp.predict(xd[:n], od[:n])
        torch.cuda.synchronize()
        od = od.cpu().numpy()
        np.testing.assert_array_equal(od[:n], got)
        assert (od[n:] == -7.0).all()
    print(f"k_predict {'-'.join(map(str, dims))}: max |p - fp64 forward| {worst:.3e}")


# ------------------------------------------------------------------ k_mlpw (bf16)
@pytest.mark.parametrize("dims", [(756, 144, 256, 2), (756, 144, 272, 2),
                                  (756, 512, 512, 256, 2)])
def test_bf16_wide_classifier_with_biases(dims):
    """k_mlpw's two- and four-column-tile instances (hidden max 256 / 272 and 512) with
    non-zero biases in every layer: f1 of mv_evaluate against the numpy restatement of the bf16
    arithmetic (tests/bf16_ref.py, variant A) at 4 x the floor measured on these rows
    (tests/test_gpu_bf16_routes.py's rule; never above the earlier 2e-3), f2 / f3 identical to
    the fp32 mode's."""
    from moeva2_amd.problem import get_engine

    p, c, sc = _project("botnet")
    W, bs = _net(dims, 61)
    eng = get_engine(c, _classifier(W, bs), sc, 2)
    mut = np.asarray(eng.prog.mut_feats)
    X = p.x[:3]
    bounds = [c.get_feature_min_max(dynamic_input=x) for x in X]
    eng.set_states(X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]), 1)
    n = 37
    probs = [p.problem(X[b]) for b in range(3)]
    genes = _perturbed_genes(p, probs, n, np.random.default_rng(62))
    gd = torch.as_tensor(genes, device="cuda")
    F32 = torch.empty((3, n, 3), dtype=torch.float64, device="cuda")
    F16 = torch.empty_like(F32)
    try:
        eng.set_mlp_precision("fp32")
        assert eng.kernel_times()["mlp_kernel"] == "k_mlpw32"
        eng.evaluate(gd, F32)
        eng.set_mlp_precision("bf16")
        assert eng.kernel_times()["mlp_kernel"] == "k_mlpw"
        eng.evaluate(gd, F16)
        torch.cuda.synchronize()
        F32, F16 = F32.cpu().numpy(), F16.cpu().numpy()
        np.testing.assert_array_equal(F16[:, :, 1:], F32[:, :, 1:])
        worst = 0.0
        for b in range(3):
            x_ml = mo.genetic_to_ml(p.lay, genes[b], X[b]) * p.ml[0] + p.ml[1]
            emu, floor = bf16_ref.f1_with_floor(x_ml, mut, W, bs, 1)
            err = float(np.abs(F16[b, :, 0] - emu).max())
            print(f"  k_mlpw {'-'.join(map(str, dims))}, state {b}: floor {floor:.3e}, "
                  f"|device - A| {err:.3e}")
            worst = max(worst, err)
            assert err <= min(2e-3, 4 * floor), (b, err, floor)
        print(f"k_mlpw {'-'.join(map(str, dims))}: max |f1 - bf16 restatement| {worst:.3e}")
    finally:
        eng.set_mlp_precision("fp32")
