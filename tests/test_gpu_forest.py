"""Tree ensembles on the device (csrc/forest.hip k_forest) against the restatement of
scikit-learn's predict_proba (moeva2_amd/models/forest.py predict_proba_numpy).

There is no tolerance on a probability or on f1: the device performs the restatement's fp64
operations in its order, so any difference is a bug.  f2 / f3 of mv_evaluate are the row
kernels' and stay bit-identical to the oracle in the engine's order.  The attack tests hold the
device loop against the hosted loop (the same forest behind a predict_proba-only wrapper): with
bit-equal f1 both loops give the same populations."""
import os

import numpy as np
import pytest

import synth_problem as sp
from oracle import device_order as do
from oracle import moeva_oracle as mo
from oracle.problems import PROJECTS, Project

from moeva2_amd.models.forest import ForestTables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "moeva2-ijcai22-replication_amd", "resources")
FOREST_ROWS = 8
ROWS = (1, 63, 64, 65, 257)  # one lane per row: the wave / workgroup edges


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class OnlyProba:
    """The same forest as a model the engine cannot compile: the hosted loop."""

    def __init__(self, tables):
        self.tables = tables

    def predict_proba(self, x):
        return self.tables.predict_proba_numpy(x)


# ---------------------------------------------------------------- forests
def random_forest(rng, x_ml, feats, n_trees, depth, n_classes=2):
    """Random trees in depth-first order over the features ``feats`` (taken in turn, so each is
    split on); every threshold is the float32 value of a row of x_ml at that feature, so rows
    sit exactly on thresholds (<= against <)."""
    x32 = np.asarray(x_ml, np.float32)
    feature, thr, left, right, roots, leaves = [], [], [], [], [], []
    turn = [0]

    def grow(d):
        i = len(feature)
        feature.append(0), thr.append(0.0), left.append(-1), right.append(-1)
        if d == 0 or (d < depth and rng.random() < 0.15):
            v = rng.integers(0, 20, n_classes).astype(np.float64)
            s = v.sum()
            leaves.append(v / (s if s != 0 else 1.0))
            feature[i] = -len(leaves)
            return i
        f = int(feats[turn[0] % len(feats)])
        turn[0] += 1
        feature[i] = f
        thr[i] = float(x32[rng.integers(0, x32.shape[0]), f])
        left[i] = grow(d - 1)
        right[i] = grow(d - 1)
        return i

    for _ in range(n_trees):
        roots.append(len(feature))
        grow(depth)
    return ForestTables.from_arrays(x32.shape[1], feature, thr, left, right, roots, leaves)


def chain(depth, go_left, d=3):
    """One tree that is a chain of ``depth`` inner nodes on feature 0, continuing on the left
    (thresholds falling: x <= -k) or on the right (rising: x > k), a distinct leaf at every
    exit, so a row's depth is its |x[0]|."""
    feature, thr, left, right, leaves = [], [], [], [], []
    n = 2 * depth + 1
    for k in range(depth):
        feature.append(0)
        thr.append(float(-k) if go_left else float(k))
        nxt, leaf = 2 * k + 2, 2 * k + 1
        if k == depth - 1:
            nxt = n - 1
        left.append(nxt if go_left else leaf)
        right.append(leaf if go_left else nxt)
        feature.append(-(len(leaves) + 1)), thr.append(0.0), left.append(-1), right.append(-1)
        leaves.append([k / (k + 1.0), 1.0 / (k + 1.0)])
    feature.append(-(len(leaves) + 1)), thr.append(0.0), left.append(-1), right.append(-1)
    leaves.append([0.125, 0.875])
    return ForestTables.from_arrays(d, feature, thr, left, right, [0], leaves)


def predict_forests():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(300, 7))
    v = np.float32(0.3)
    out = {
        # a root that is a leaf, next to a real tree
        "root_only": ForestTables.from_arrays(7, [-1, 0, -2, -3], [0, 0.1, 0, 0], [-1, 2, -1, -1],
                                              [-1, 3, -1, -1], [0, 1],
                                              [[0.25, 0.75], [1.0, 0.0], [0.0, 1.0]]),
        # depth 1, the threshold equal to a row's float32 value: that row goes left
        "equal_threshold": ForestTables.from_arrays(7, [2, -1, -2], [float(v), 0, 0], [1, -1, -1],
                                                    [2, -1, -1], [0], [[0.9, 0.1], [0.2, 0.8]]),
        "left_chain_40": chain(40, True, 7),
        "right_chain_40": chain(40, False, 7),
        "classes_8": random_forest(rng, x, range(7), 5, 6, n_classes=8),
        "one_tree": random_forest(rng, x, range(7), 1, 7),
        "trees_33": random_forest(rng, x, range(7), 33, 6, n_classes=3),
    }
    return out, v


@pytest.mark.parametrize("name", ["root_only", "equal_threshold", "left_chain_40",
                                  "right_chain_40", "classes_8", "one_tree", "trees_33"])
def test_forest_predict_bit_exact(name):
    from moeva2_amd import _native

    forests, v = predict_forests()
    t = forests[name]
    f = _native.Forest(t)
    rng = np.random.default_rng(17)
    for n in ROWS:
        x = rng.normal(size=(n, 7))
        x[:, 0] = rng.uniform(-45, 45, n)  # the chains' exits
        x[0, 2] = float(v)                      # exactly on equal_threshold's split
        if n > 1:
            x[1, 2] = float(np.nextafter(v, np.float32(1)))
            x[n // 2, 0] = np.round(x[n // 2, 0])  # on a chain threshold
        xd = torch.as_tensor(x, device="cuda")
        out = torch.empty((n, t.n_classes), dtype=torch.float64, device="cuda")
        f.predict(xd, out)
        torch.cuda.synchronize()
        want = t.predict_proba_numpy(x)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{name}, {n} rows")
        if name == "equal_threshold":
            assert want[0, 0] == 0.9 and (n == 1 or want[1, 0] == 0.2)


# ---------------------------------------------------------------- engine
class NpScaler:
    def __init__(self, scale, mn):
        self.scale_, self.min_ = np.asarray(scale, np.float64), np.asarray(mn, np.float64)


class Lcld:
    """The shipped LCLD problem with the handles of a synthetic case."""

    name = "lcld"

    def __init__(self):
        from moeva2_amd.experiments.united.utils import STR_TO_CONSTRAINTS_CLASS
        from moeva2_amd.problem import build_device_program

        self.p = Project("lcld")
        feat = os.path.join(RES, PROJECTS["lcld"][0])
        self.constraints = STR_TO_CONSTRAINTS_CLASS["lcld"](feat, feat.replace("features",
                                                                                "constraints"))
        d = np.load(os.path.join(RES, PROJECTS["lcld"][2]))
        self.ml = (np.asarray(d["scale_"], np.float64), np.asarray(d["min_"], np.float64))
        self.scaler = NpScaler(*self.ml)
        self.X = self.p.x[:sp.B].copy()
        self.lay = self.p.lay
        self.probs = [self.p.problem(x) for x in self.X]
        self.codes = build_device_program(self.constraints).op_code

    def bounds(self):
        b = [self.constraints.get_feature_min_max(dynamic_input=x) for x in self.X]
        return np.array([v[0] for v in b]), np.array([v[1] for v in b])

    def eval_genes(self, rng):
        isr = np.array([t == "real" for t in mo.genetic_types(self.lay)])
        genes = []
        for prob in self.probs:
            gl, gu = mo.genetic_bounds(self.lay, prob.xl, prob.xu)
            g = np.repeat(mo.initial_population(prob, 1), 37, axis=0)
            for r in range(1, 37):
                k = rng.integers(0, self.lay.V, size=1 + r % 5)
                v = rng.uniform(gl[k], gu[k])
                g[r, k] = np.where(isr[k], v, np.round(v))
            genes.append(g)
        return np.stack(genes)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("forest_synth")
    cache = {}

    def get(name):
        if name not in cache:
            sy = Lcld() if name == "lcld" else sp.build(name, d)
            if name != "lcld":
                sy.name = name
            sy.forest = case_forest(sy)
            cache[name] = sy
        return cache[name]

    return get


def ml_rows(sy, b, genes):
    return mo.genetic_to_ml(sy.lay, genes, sy.probs[b].x_init) * sy.ml[0] + sy.ml[1]


def eval_rows(sy):
    g = sy.eval_genes(np.random.default_rng(23))
    g = g[0] if isinstance(g, tuple) else g
    # finite rows only: the synthetic cases end with rows that hold an infinite gene
    keep = np.isfinite(g).all(axis=(0, 2))
    return np.ascontiguousarray(g[:, keep])


def case_forest(sy):
    """9 random trees of depth 6 over: mutable plain features, immutable features, one-hot
    columns where the problem has them, and -- the compact cases -- features of genes the
    MLP engine's compact layout would fix.  Thresholds come from the ML rows the test
    evaluates, so rows lie on thresholds."""
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
    fixed = do.compact_fixed(lay, sy.probs) if sy.name.startswith("k_") else None
    if fixed is not None and fixed.any():
        ff = np.where(fixed)[0]
        feats += list(rng.choice(ff, 3, replace=False))
        groups["fixed"] = set(ff.tolist())
    rng.shuffle(feats)
    t = random_forest(rng, x, feats, 9, 6)
    used = set(t.feature[t.feature >= 0].tolist())
    for what, fs in groups.items():
        assert used & fs, f"{sy.name}: no split on a {what} feature"
    return t


def forest_engine(sy, tables=None, mc=1):
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.problem import get_engine

    if not hasattr(sy, "clf"):
        sy.clf = Classifier(sy.forest)
    eng = get_engine(sy.constraints, sy.clf, sy.scaler, 2)
    xl, xu = sy.bounds()
    eng.set_states(sy.X, xl, xu, mc)
    return eng


@pytest.mark.parametrize("name", ["lcld", "n8p", "g33", "n32d", "c129", "k_slab"])
def test_evaluate_f1_bit_exact(cases, name):
    sy = cases(name)
    mc = np.array([1, 0, 1])
    eng = forest_engine(sy, mc=mc)
    assert eng.mlp_kernel() == FOREST_ROWS
    # the forest engine keeps the full gene layout, compact cases included
    assert eng.stored_genes().all()
    genes = eval_rows(sy)
    n = genes.shape[1]
    F = torch.empty((sp.B, n, 3), dtype=torch.float64, device="cuda")
    eng.evaluate(torch.as_tensor(genes, device="cuda"), F)
    torch.cuda.synchronize()
    F = F.cpu().numpy()
    for b, prob in enumerate(sy.probs):
        what = f"{name}, state {b}"
        want = sy.forest.predict_proba_numpy(ml_rows(sy, b, genes[b]))[:, mc[b]]
        np.testing.assert_array_equal(F[b, :, 0], want, err_msg=what)
        ref = do.evaluate_device_order(prob, genes[b], sy.codes)
        np.testing.assert_array_equal(F[b, :, 1], ref[:, 1], err_msg=what)
        if getattr(getattr(sy, "case", None), "install", False) or name == "lcld":
            np.testing.assert_allclose(F[b, :, 2], ref[:, 2], rtol=1e-14, atol=0, err_msg=what)
        else:
            np.testing.assert_array_equal(F[b, :, 2], ref[:, 2], err_msg=what)
    assert np.unique(F[:, :, 0]).size > 3, "the forest does not tell these rows apart"


def attack(sy, model, mc, seed=7, streams=False, X=None, first_state=0, crossover="two_point"):
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2

    m = Moeva2(model, sy.constraints, ml_scaler=sy.scaler, norm=2, n_gen=5, n_pop=37,
               n_offsprings=20, save_history="full", seed=seed, state_streams=streams,
               crossover=crossover)
    X = sy.X if X is None else X
    g, F, h = m.generate(X, mc, return_device=True, first_state=first_state)
    torch.cuda.synchronize()
    return m, g.cpu().numpy(), F.cpu().numpy(), h.cpu().numpy()


@pytest.mark.parametrize("name", ["lcld", "c129"])
@pytest.mark.parametrize("mc", [1, (1, 0, 1)], ids=["class1", "classes101"])
def test_attack_device_loop_equals_hosted_loop(cases, name, mc):
    sy = cases(name)
    mc = np.asarray(mc) if isinstance(mc, tuple) else mc
    md, gd, Fd, hd = attack(sy, sy.forest, mc)
    assert md.last_engine.mlp_kernel() == FOREST_ROWS
    mh, gh, Fh, hh = attack(sy, OnlyProba(sy.forest), mc)
    assert mh.last_engine.mlp_kernel() == -1  # the hosted loop
    assert hd.shape == (sp.B, 40 + 4 * 20, 3 + md.last_engine.prog.C)
    np.testing.assert_array_equal(hd, hh)
    np.testing.assert_array_equal(gd, gh)
    np.testing.assert_array_equal(Fd, Fh)
    assert np.unique(hd[:, :, 0]).size > 3 and (gd != gd[:, :1]).any()


def test_attack_sbx_device_loop_equals_hosted_loop(cases):
    sy = cases("n8p")
    _, gd, Fd, hd = attack(sy, sy.forest, 1, crossover="sbx")
    _, gh, Fh, hh = attack(sy, OnlyProba(sy.forest), 1, crossover="sbx")
    np.testing.assert_array_equal(hd, hh)
    np.testing.assert_array_equal(gd, gh)
    np.testing.assert_array_equal(Fd, Fh)


def test_state_streams_state_equals_its_own_run(cases):
    sy = cases("lcld")
    _, g3, F3, h3 = attack(sy, sy.forest, 1, streams=True)
    for b in range(sp.B):
        _, g1, F1, h1 = attack(sy, sy.forest, 1, streams=True, X=sy.X[b:b + 1], first_state=b)
        np.testing.assert_array_equal(g1[0], g3[b])
        np.testing.assert_array_equal(F1[0], F3[b])
        np.testing.assert_array_equal(h1[0], h3[b])
    assert (g3[0] != g3[1]).any()


def test_objective_calculator_forest_equals_host_scoring(cases):
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator

    sy = cases("lcld")
    m, g, _, _ = attack(sy, sy.forest, 1)
    x_f = np.stack([m._encoder.genetic_to_ml(g[b], sy.X[b]) for b in range(sp.B)])
    thr = {"f1": 0.5, "f2": 4.0}
    dev = ObjectiveCalculator(Classifier(sy.forest), sy.constraints, 1, thr,
                              min_max_scaler=sy.scaler, ml_scaler=sy.scaler, norm=2)
    host = ObjectiveCalculator(Classifier(OnlyProba(sy.forest)), sy.constraints, 1, thr,
                               min_max_scaler=sy.scaler, ml_scaler=sy.scaler, norm=2)
    assert type(dev._device()[2]).__name__ == "Forest" and host._device()[2] is None
    od, oh = dev.calculate_objectives_3d(sy.X, x_f), host.calculate_objectives_3d(sy.X, x_f)
    # no candidate sits on the classification threshold: none is excluded
    assert (np.abs(od[..., 1] - thr["f1"]) > 1e-9).all()
    np.testing.assert_array_equal(od, oh)
    want = sy.forest.predict_proba_numpy(
        (x_f.reshape(-1, x_f.shape[2]) * sy.ml[0] + sy.ml[1]))[:, 1].reshape(sp.B, -1)
    np.testing.assert_array_equal(od[..., 1], want)
    for b in range(sp.B):
        np.testing.assert_array_equal(dev._objective_respected(od[b]),
                                      host._objective_respected(oh[b]))
    np.testing.assert_array_equal(dev.success_rate_3d(sy.X, x_f), host.success_rate_3d(sy.X, x_f))
    # and on device tensors (generate_scored_sharded's path)
    xi, xd = torch.as_tensor(sy.X, device="cuda"), torch.as_tensor(x_f, device="cuda")
    np.testing.assert_array_equal(dev.calculate_objectives_device(xi, xd).cpu().numpy(), od)


def test_refusals(cases):
    from moeva2_amd import _native
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.io.tf_bundle import DenseMLP
    from moeva2_amd.problem import get_engine

    sy = cases("n8p")
    m = Moeva2(sy.forest, sy.constraints, ml_scaler=sy.scaler, norm=2, n_gen=2, n_pop=37,
               n_offsprings=20, seed=1, mlp_dtype="bf16")
    with pytest.raises(ValueError):
        m.generate(sy.X, 1)
    # an engine that has an MLP
    mlp = Classifier(DenseMLPModel(DenseMLP(sy.W, sy.bs, ["relu", "relu", "softmax"])))
    eng = get_engine(sy.constraints, mlp, sy.scaler, 2)
    with pytest.raises(_native.NativeError, match="error 3"):
        eng.set_forest(sy.forest)
    assert eng.forest is None and eng.mlp_kernel() != FOREST_ROWS
    # after mv_set_states, and a second forest
    hosted = get_engine(sy.constraints, Classifier(OnlyProba(sy.forest)), sy.scaler, 2)
    xl, xu = sy.bounds()
    hosted.set_states(sy.X, xl, xu, 1)
    with pytest.raises(_native.NativeError, match="error 3"):
        hosted.set_forest(sy.forest)
    assert hosted.mlp_kernel() == -1
    with pytest.raises(_native.NativeError, match="error 3"):
        forest_engine(sy).set_forest(sy.forest)
    # a forest of another width
    other = ForestTables.from_arrays(sy.forest.n_features + 1, [-1], [0.0], [-1], [-1], [0],
                                     [[0.5, 0.5]])
    fresh = _native.Engine(hosted.prog, None, None)
    with pytest.raises(ValueError):
        fresh.set_forest(other)
    # minimize_class outside the forest's classes
    with pytest.raises(_native.NativeError):
        forest_engine(sy, mc=2)
