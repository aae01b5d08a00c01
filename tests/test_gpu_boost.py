"""Gradient-boosted ensembles on the device (csrc/boost.hip k_boost) against the restatement of
scikit-learn's predict_proba (moeva2_amd/models/boost.py predict_proba_numpy).

There is no tolerance on a probability or on f1: the device performs the restatement's fp64
operations in its order with the same exp (csrc/detmath.h, whose host build the restatement
calls), so any difference is a bug.  Both routes are held to it: k_boost walking a
per-workgroup LDS copy of the nodes (kind 10: the packed nodes fit 64 KiB = 4,096 nodes) and
k_boost reading them from global memory (kind 9).  The attack tests hold the device loop
against the hosted loop (the same ensemble's restatement behind a predict_proba-only wrapper):
with bit-equal f1 both loops give the same populations."""
import numpy as np
import pytest

import synth_problem as sp
from oracle import device_order as do
from test_gpu_forest import Lcld, eval_rows, ml_rows

from moeva2_amd.models.boost import BoostModel, BoostTables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOOST_ROWS, BOOST_ROWS_LDS = 9, 10
LDS_NODES = 4096  # csrc/boost.h BOOST_LDS_MAX_BYTES / 16
# one lane per row: the wave edges (the global-memory route's workgroup) and the LDS route's
# workgroup of 256
ROWS = (1, 63, 64, 65, 255, 256, 257)
D = 7


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class OnlyProba:
    """The same ensemble as a model the engine cannot compile: the hosted loop."""

    def __init__(self, tables):
        self.tables = tables

    def predict_proba(self, x):
        return self.tables.predict_proba_numpy(x)


# ---------------------------------------------------------------- ensembles
def random_boost(rng, x_ml, feats, n_stages, depth, n_classes=2, p_leaf=0.15, amp=1.0):
    """Random trees in depth-first order over the features ``feats`` (taken in turn), stage
    major; every threshold is the float32 value of a row of x_ml at that feature, so rows sit
    exactly on thresholds (<= against <).  p_leaf = 0: full trees of 2^(depth + 1) - 1 nodes."""
    x32 = np.asarray(x_ml, np.float32)
    feature, thr, left, right, roots, leaves = [], [], [], [], [], []
    turn = [0]

    def grow(d):
        i = len(feature)
        feature.append(0), thr.append(0.0), left.append(-1), right.append(-1)
        if d == 0 or (d < depth and rng.random() < p_leaf):
            leaves.append(float(rng.normal()) * amp)
            feature[i] = -len(leaves)
            return i
        f = int(feats[turn[0] % len(feats)])
        turn[0] += 1
        feature[i] = f
        thr[i] = float(x32[rng.integers(0, x32.shape[0]), f])
        left[i] = grow(d - 1)
        right[i] = grow(d - 1)
        return i

    n_out = 1 if n_classes == 2 else n_classes
    for _ in range(n_stages * n_out):
        roots.append(len(feature))
        grow(depth)
    return BoostTables.from_arrays(x32.shape[1], n_classes, feature, thr, left, right, roots,
                                   leaves, rng.normal(size=n_out))


def with_root_only_trees(t, n_extra, rng):
    """t plus n_extra trees that are a single leaf (appended; n_extra a multiple of n_outputs)."""
    n, nl = t.n_nodes, t.n_leaves
    k = np.arange(n_extra)
    return BoostTables.from_arrays(
        t.n_features, t.n_classes, np.concatenate([t.feature, -(nl + k) - 1]),
        np.concatenate([t.threshold, np.zeros(n_extra)]),
        np.concatenate([t.left, np.full(n_extra, -1)]),
        np.concatenate([t.right, np.full(n_extra, -1)]), np.concatenate([t.tree_root, n + k]),
        np.concatenate([t.leaf_value, rng.normal(size=n_extra) * 0.01]), t.base)


def predict_cases():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(300, D))
    v = np.float32(0.3)
    full3 = lambda stages, k: random_boost(rng, x, range(D), stages, 3, k, p_leaf=0.0, amp=0.05)
    out = {
        # a root that is a leaf, next to a real tree (K = 2: every tree adds to raw[0])
        "root_only": BoostTables.from_arrays(D, 2, [-1, 0, -2, -3], [0, 0.1, 0, 0],
                                             [-1, 2, -1, -1], [-1, 3, -1, -1], [0, 1],
                                             [0.25, -1.5, 0.75], [0.125]),
        "one_tree": random_boost(rng, x, range(D), 1, 3),
        # depth 1, the threshold equal to a row's float32 value: that row goes left
        "equal_threshold": BoostTables.from_arrays(D, 2, [2, -1, -2], [float(v), 0, 0],
                                                   [1, -1, -1], [2, -1, -1], [0], [2.0, -2.0],
                                                   [0.0]),
        "depth1_k3": random_boost(rng, x, range(D), 5, 1, 3, p_leaf=0.0),
        "depth6_k8": random_boost(rng, x, range(D), 3, 6, 8),
        "depth6_k2": random_boost(rng, x, range(D), 9, 6, 2),
        # raw scores of -800, -40, 40, 800 by x[0] in (.., -1], (-1, 0], (0, 1], (1, ..): the
        # sigmoid saturates, E overflows to inf (p1 = 1 / inf = 0) and underflows to 0 (p1 = 1)
        "sigmoid_saturates": BoostTables.from_arrays(
            D, 2, [0, 0, 0, -1, -2, -3, -4], [0.0, -1.0, 1.0, 0, 0, 0, 0],
            [1, 3, 5, -1, -1, -1, -1], [2, 4, 6, -1, -1, -1, -1], [0],
            [-800.0, -40.0, 40.0, 800.0], [0.0]),
        # K = 3, one stage: class 0 at 800 or 0 by x[0], class 1 at 1, class 2 at -735 (E gives a
        # subnormal) or 40 by x[1]: one class far above the rest, E underflowing to 0
        "softmax_far": BoostTables.from_arrays(
            D, 3, [0, -1, -2, -3, 1, -4, -5], [0.0, 0, 0, 0, 0.0, 0, 0],
            [1, -1, -1, -1, 5, -1, -1], [2, -1, -1, -1, 6, -1, -1], [0, 3, 4],
            [800.0, 0.0, 1.0, -735.0, 40.0], [0.0, 0.0, 0.0]),
    }
    # 273 full depth-3 trees are 4,095 nodes: with one root-only tree the budget exactly (the
    # LDS route's last size), with two one node over (the global-memory route's first)
    out["at_lds_budget"] = with_root_only_trees(full3(273, 2), 1, rng)
    out["over_lds_budget"] = with_root_only_trees(full3(273, 2), 2, rng)
    assert out["at_lds_budget"].n_nodes == LDS_NODES
    assert out["over_lds_budget"].n_nodes == LDS_NODES + 1
    return out, v


_PREDICT = {}


def predict_case(name):
    if not _PREDICT:
        _PREDICT["cases"], _PREDICT["v"] = predict_cases()
    return _PREDICT["cases"][name], _PREDICT["v"]


@pytest.mark.parametrize("name", ["root_only", "one_tree", "equal_threshold", "depth1_k3",
                                  "depth6_k8", "depth6_k2", "sigmoid_saturates", "softmax_far",
                                  "at_lds_budget", "over_lds_budget"])
def test_boost_predict_bit_exact(name):
    """mv_forest_predict on a boost handle (the LDS route up to 4,096 packed nodes, the
    global-memory route past them) equals predict_proba_numpy bit for bit."""
    from moeva2_amd import _native

    t, v = predict_case(name)
    f = _native.Boost(t)
    assert isinstance(f, _native.Forest)  # the forest handle
    rng = np.random.default_rng(17)
    seen = set()
    for n in ROWS:
        x = rng.normal(size=(n, D))
        x[:, 0] = rng.uniform(-2, 2, n)
        x[0, 2] = float(v)  # exactly on equal_threshold's split
        if n > 1:
            x[1, 2] = float(np.nextafter(v, np.float32(1)))
            x[n // 2, 0] = np.round(x[n // 2, 0])  # on a threshold of the saturating trees
        xd = torch.as_tensor(x, device="cuda")
        out = torch.empty((n, t.n_classes), dtype=torch.float64, device="cuda")
        f.predict(xd, out)
        torch.cuda.synchronize()
        want = t.predict_proba_numpy(x)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{name}, {n} rows")
        seen.update(np.unique(want).tolist())
        if name == "equal_threshold":
            assert want[0, 1] > 0.5 and (n == 1 or want[1, 1] < 0.5)
    if name == "sigmoid_saturates":
        assert 0.0 in seen and 1.0 in seen and any(0.0 < p < 1e-15 for p in seen)
    if name == "softmax_far":
        assert 0.0 in seen and 1.0 in seen and any(0.0 < p < 1e-300 for p in seen)


def test_boost_model_predicts_on_the_device():
    t, _ = predict_case("depth6_k8")
    x = np.random.default_rng(3).normal(size=(130, D))
    np.testing.assert_array_equal(BoostModel(t).predict_proba(x), t.predict_proba_numpy(x))


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("boost_synth")
    cache = {}

    def get(name):
        if name not in cache:
            sy = Lcld() if name == "lcld" else sp.build(name, d)
            if name != "lcld":
                sy.name = name
            sy.boost = {}
            cache[name] = sy
        return cache[name]

    return get


def case_boost(sy, kind):
    """Random stages over mutable plain features (read from the ML row), immutable features
    (read from xfix) and one-hot columns where the problem has them; thresholds come from the
    ML rows the test evaluates, so rows lie on thresholds.
      lds2 / lds3: 12 stages of depth 3, two / three classes: the LDS route
      l2:          33 stages of full depth-6 trees (4,191 nodes > 4,096): the global-memory route"""
    if kind in sy.boost:
        return sy.boost[kind]
    lay = sy.lay
    mut = np.where(lay.mutable_mask)[0]
    imm = np.where(~lay.mutable_mask)[0]
    genes = eval_rows(sy)
    x = np.concatenate([ml_rows(sy, b, genes[b]) for b in range(sp.B)])
    rng = np.random.default_rng(31)
    feats = list(rng.choice(mut, min(6, mut.size), replace=False))
    feats += list(rng.choice(imm, min(3, imm.size), replace=False))
    groups = {"mutable": set(mut.tolist()), "immutable": set(imm.tolist())}
    types = np.asarray(getattr(sy, "types", None) if hasattr(sy, "types")
                       else sy.constraints.get_feature_type())
    ohe = [f for f in mut if str(types[f]).startswith("ohe")]
    if ohe:
        feats += list(rng.choice(ohe, min(3, len(ohe)), replace=False))
        groups["one-hot"] = set(ohe)
    rng.shuffle(feats)
    if kind == "l2":
        t = random_boost(rng, x, feats, 33, 6, 2, p_leaf=0.0, amp=0.2)
        assert t.n_nodes > LDS_NODES
    else:
        t = random_boost(rng, x, feats, 12, 3, 2 if kind == "lds2" else 3, amp=0.5)
        assert t.n_nodes <= LDS_NODES
    used = set(t.feature[t.feature >= 0].tolist())
    for what, fs in groups.items():
        assert used & fs, f"{sy.name}: no split on a {what} feature"
    sy.boost[kind] = t
    return t


def boost_engine(sy, tables, mc=1):
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.problem import get_engine

    eng = get_engine(sy.constraints, Classifier(tables), sy.scaler, 2)
    xl, xu = sy.bounds()
    eng.set_states(sy.X, xl, xu, mc)
    return eng


@pytest.mark.parametrize("kind,route", [("lds2", BOOST_ROWS_LDS), ("lds3", BOOST_ROWS_LDS),
                                        ("l2", BOOST_ROWS)])
@pytest.mark.parametrize("name", ["lcld", "n8p", "c129"])
def test_evaluate_f1_bit_exact(cases, name, kind, route):
    """mv_evaluate's F[..][0] on both routes: splits on mutable features (the fp32 ML row) and on
    features the attack does not move (xfix), min_class 0 and K - 1 in one batch."""
    sy = cases(name)
    t = case_boost(sy, kind)
    top = t.n_classes - 1
    mc = np.array([top, 0, top])
    eng = boost_engine(sy, t, mc=mc)
    assert eng.mlp_kernel() == route
    assert eng.stored_genes().all()  # the full gene layout, as with a forest
    genes = eval_rows(sy)
    n = genes.shape[1]
    F = torch.empty((sp.B, n, 3), dtype=torch.float64, device="cuda")
    eng.evaluate(torch.as_tensor(genes, device="cuda"), F)
    torch.cuda.synchronize()
    F = F.cpu().numpy()
    for b, prob in enumerate(sy.probs):
        what = f"{name}, {kind}, state {b}"
        want = t.predict_proba_numpy(ml_rows(sy, b, genes[b]))[:, mc[b]]
        np.testing.assert_array_equal(F[b, :, 0], want, err_msg=what)
        ref = do.evaluate_device_order(prob, genes[b], sy.codes)
        np.testing.assert_array_equal(F[b, :, 1], ref[:, 1], err_msg=what)
    assert np.unique(F[:, :, 0]).size > 3, "the ensemble does not tell these rows apart"


def attack(sy, model, mc, seed=7, streams=False, X=None, first_state=0, crossover="two_point",
           history="full"):
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2

    m = Moeva2(model, sy.constraints, ml_scaler=sy.scaler, norm=2, n_gen=5, n_pop=37,
               n_offsprings=20, save_history=history, seed=seed, state_streams=streams,
               crossover=crossover)
    X = sy.X if X is None else X
    out = m.generate(X, mc, return_device=True, first_state=first_state)
    torch.cuda.synchronize()
    return (m,) + tuple(None if o is None else o.cpu().numpy() for o in out)


def fitted_gb(sy, n_classes=2):
    """A small GradientBoostingClassifier fitted on the problem's ML rows."""
    from sklearn.ensemble import GradientBoostingClassifier

    key = ("gb", n_classes)
    if key not in sy.boost:
        rng = np.random.default_rng(0)
        xm = sy.p.x[:400] * sy.ml[0] + sy.ml[1]
        xm = np.clip(xm + rng.normal(0.0, 0.05, xm.shape), 0.0, 1.0)
        s = xm @ rng.normal(size=xm.shape[1]) + 0.5 * np.sin(7.0 * xm[:, 0])
        y = np.digitize(s, np.quantile(s, np.arange(1, n_classes) / n_classes))
        sy.boost[key] = GradientBoostingClassifier(n_estimators=10, max_depth=3,
                                                   random_state=0).fit(xm, y)
    return sy.boost[key]


@pytest.mark.parametrize("n_classes,mc", [(2, 1), (3, (2, 0, 2))], ids=["k2", "k3_classes202"])
def test_attack_fitted_gb_device_loop_equals_hosted_loop(cases, n_classes, mc):
    """Moeva2.generate with a fitted GradientBoostingClassifier, full history: the device loop
    (offspring f1 written through out_map, the history's f1 column) against the hosted loop
    driven by the restatement."""
    sy = cases("lcld")
    gb = fitted_gb(sy, n_classes)
    t = BoostTables.from_sklearn(gb)
    mc = np.asarray(mc) if isinstance(mc, tuple) else mc
    md, gd, Fd, hd = attack(sy, gb, mc)
    assert md.last_engine.mlp_kernel() == BOOST_ROWS_LDS
    mh, gh, Fh, hh = attack(sy, OnlyProba(t), mc)
    assert mh.last_engine.mlp_kernel() == -1  # the hosted loop
    assert hd.shape == (sp.B, 40 + 4 * 20, 3 + md.last_engine.prog.C)
    np.testing.assert_array_equal(hd, hh)
    np.testing.assert_array_equal(gd, gh)
    np.testing.assert_array_equal(Fd, Fh)
    assert np.unique(hd[:, :, 0]).size > 3 and (gd != gd[:, :1]).any()
    # the final f1 is the restatement of the decoded final population
    for b in range(sp.B):
        want = t.predict_proba_numpy(ml_rows(sy, b, gd[b]))[:, np.broadcast_to(mc, sp.B)[b]]
        np.testing.assert_array_equal(Fd[b, :, 0], want)


def test_attack_global_memory_route_and_sbx(cases):
    sy = cases("n8p")
    t = case_boost(sy, "l2")
    md, gd, Fd, hd = attack(sy, t, 1, crossover="sbx")
    assert md.last_engine.mlp_kernel() == BOOST_ROWS
    _, gh, Fh, hh = attack(sy, OnlyProba(t), 1, crossover="sbx")
    np.testing.assert_array_equal(hd, hh)
    np.testing.assert_array_equal(gd, gh)
    np.testing.assert_array_equal(Fd, Fh)


def test_state_streams_state_equals_its_own_run(cases):
    sy = cases("lcld")
    gb = fitted_gb(sy)
    _, g3, F3, h3 = attack(sy, gb, 1, streams=True)
    for b in range(sp.B):
        _, g1, F1, h1 = attack(sy, gb, 1, streams=True, X=sy.X[b:b + 1], first_state=b)
        np.testing.assert_array_equal(g1[0], g3[b])
        np.testing.assert_array_equal(F1[0], F3[b])
        np.testing.assert_array_equal(h1[0], h3[b])
    assert (g3[0] != g3[1]).any()


def test_objective_calculator_and_generate_scored(cases):
    """ObjectiveCalculator with a BoostModel equals the host computation, and
    generate_scored_sharded's verdict is the one scored from generate's populations."""
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator

    sy = cases("lcld")
    gb = fitted_gb(sy)
    t = BoostTables.from_sklearn(gb)
    m, g, _, _ = attack(sy, gb, 1, history=None)
    x_f = np.stack([m._encoder.genetic_to_ml(g[b], sy.X[b]) for b in range(sp.B)])
    thr = {"f1": 0.5, "f2": 4.0}
    dev = ObjectiveCalculator(Classifier(BoostModel(t)), sy.constraints, 1, thr,
                              min_max_scaler=sy.scaler, ml_scaler=sy.scaler, norm=2)
    host = ObjectiveCalculator(Classifier(OnlyProba(t)), sy.constraints, 1, thr,
                               min_max_scaler=sy.scaler, ml_scaler=sy.scaler, norm=2)
    assert type(dev._device()[2]).__name__ == "Boost" and host._device()[2] is None
    od, oh = dev.calculate_objectives_3d(sy.X, x_f), host.calculate_objectives_3d(sy.X, x_f)
    # no candidate sits on the classification threshold: none is excluded
    assert (np.abs(od[..., 1] - thr["f1"]) > 1e-9).all()
    np.testing.assert_array_equal(od, oh)
    want = t.predict_proba_numpy(
        (x_f.reshape(-1, x_f.shape[2]) * sy.ml[0] + sy.ml[1]))[:, 1].reshape(sp.B, -1)
    np.testing.assert_array_equal(od[..., 1], want)
    np.testing.assert_array_equal(dev.success_rate_3d(sy.X, x_f), host.success_rate_3d(sy.X, x_f))
    xi, xd = torch.as_tensor(sy.X, device="cuda"), torch.as_tensor(x_f, device="cuda")
    np.testing.assert_array_equal(dev.calculate_objectives_device(xi, xd).cpu().numpy(), od)
    # generate_scored: one process, the same seed: flags of the populations scored above
    ms = Moeva2(gb, sy.constraints, ml_scaler=sy.scaler, norm=2, n_gen=5, n_pop=37,
                n_offsprings=20, save_history=None, seed=7)
    flags, best = ms.generate_scored_sharded(sy.X, 1, dev)
    resp = np.stack([dev._objective_respected(o) for o in od])
    np.testing.assert_array_equal(flags, resp.any(axis=1))
    assert best.shape == (sp.B, sy.X.shape[1])


def test_refusals(cases):
    """mv_engine_set_boost on an engine that has a model, after mv_set_states, a second time or
    with a wrong D returns the documented error (3 = MV_ERR_STATE, ValueError for MV_ERR_ARG)."""
    from moeva2_amd import _native
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.io.tf_bundle import DenseMLP
    from moeva2_amd.problem import get_engine

    sy = cases("n8p")
    t = case_boost(sy, "lds2")
    mlp = Classifier(DenseMLPModel(DenseMLP(sy.W, sy.bs, ["relu", "relu", "softmax"])))
    eng = get_engine(sy.constraints, mlp, sy.scaler, 2)
    with pytest.raises(_native.NativeError, match="error 3"):
        eng.set_boost(t)
    assert eng.forest is None and eng.mlp_kernel() not in (BOOST_ROWS, BOOST_ROWS_LDS)
    hosted = get_engine(sy.constraints, Classifier(OnlyProba(t)), sy.scaler, 2)
    xl, xu = sy.bounds()
    hosted.set_states(sy.X, xl, xu, 1)
    with pytest.raises(_native.NativeError, match="error 3"):
        hosted.set_boost(t)
    assert hosted.mlp_kernel() == -1
    with pytest.raises(_native.NativeError, match="error 3"):
        boost_engine(sy, t).set_boost(t)
    other = BoostTables.from_arrays(t.n_features + 1, 2, [-1], [0.0], [-1], [-1], [0], [0.5],
                                    [0.0])
    fresh = _native.Engine(hosted.prog, None, None)
    with pytest.raises(ValueError):
        fresh.set_boost(other)
    assert fresh.mlp_kernel() == -1
    # minimize_class outside the ensemble's classes
    with pytest.raises(_native.NativeError):
        boost_engine(sy, t, mc=2)
    # the bf16 mode is the Dense MLP's
    with pytest.raises(ValueError):
        boost_engine(sy, t).set_mlp_precision("bf16")
