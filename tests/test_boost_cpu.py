"""Gradient-boosted ensembles without a GPU: the restatement of scikit-learn's decision_function
and predict_proba (moeva2_amd/models/boost.py), the table checks on the Python side and behind
the C ABI (they come before any device call), files, classifier detection, the exported symbols
and the routes.

Raw scores: bit-equal to sklearn's decision_function on float32-representable rows.

Probabilities: the restatement's exp is the engine's (csrc/detmath.h det_exp2, fdlibm's exp),
sklearn's is the C library's behind scipy's expit / softmax; both are sub-ulp but not correctly
rounded, so the two differ in the last bits.  Measured on the inputs below with scikit-learn
1.7.2, in units of the last place of sklearn's value: at most 2 ulps for two and three
classes, 3 (hist8) and 4 (gb8) for eight, where the softmax sums eight rounded terms; 0 where
the raw score takes few values (gb2_one_stage, gb2_zero_init, hist2_single_node).  The largest
is 4 ulps; the bound is twice that measurement, MAX_ULP = 8, fixed before any
device run.
"""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from moeva2_amd.models.boost import BoostModel, BoostTables

sklearn = pytest.importorskip("sklearn")

MAX_ULP = 8  # twice the measured maximum of 4 (module docstring)
D = 9


def _data(n, k, seed):
    """float32-representable rows, a label that depends on several features."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D)).astype(np.float32).astype(np.float64)
    y = (np.abs(X[:, 0] * 3 + X[:, 1] * X[:, 2]) * 1.7).astype(int) % k
    return X, y


KINDS = {
    # name: (family, classes, parameters)
    "gb2": ("gb", 2, dict(n_estimators=25, max_depth=3, learning_rate=0.1)),
    "gb3": ("gb", 3, dict(n_estimators=12, max_depth=4, learning_rate=0.2)),
    "gb8": ("gb", 8, dict(n_estimators=6, max_depth=3, learning_rate=0.3)),
    "gb2_one_stage": ("gb", 2, dict(n_estimators=1, max_depth=2)),
    "gb3_single_node": ("gb", 3, dict(n_estimators=3, min_samples_split=100000)),
    "gb2_zero_init": ("gb", 2, dict(n_estimators=5, max_depth=2, init="zero")),
    "hist2": ("hist", 2, dict(max_iter=25, max_depth=3, learning_rate=0.1)),
    "hist3": ("hist", 3, dict(max_iter=12, max_leaf_nodes=9, learning_rate=0.2)),
    "hist8": ("hist", 8, dict(max_iter=6, max_depth=3, learning_rate=0.3)),
    "hist3_one_stage": ("hist", 3, dict(max_iter=1, max_depth=2)),
    "hist2_single_node": ("hist", 2, dict(max_iter=3, min_samples_leaf=400)),
}
_FITTED = {}


def _fit(kind):
    from sklearn.ensemble import GradientBoostingClassifier, HistGradientBoostingClassifier

    if kind not in _FITTED:
        family, k, kw = KINDS[kind]
        X, y = _data(600, k, 7)
        if family == "gb":
            m = GradientBoostingClassifier(random_state=0, **kw)
        else:
            m = HistGradientBoostingClassifier(random_state=0, early_stopping=False, **kw)
        _FITTED[kind] = m.fit(X, y)
    return _FITTED[kind]


def _ulps(got, want):
    """|got - want| in units of the last place of want."""
    return np.abs(got - want) / np.spacing(np.abs(want))


@pytest.mark.parametrize("kind", list(KINDS))
def test_raw_scores_bit_equal_to_sklearn(kind):
    m = _fit(kind)
    family, k, _ = KINDS[kind]
    t = BoostTables.from_sklearn(m)
    assert t.n_classes == k and t.n_outputs == (1 if k == 2 else k)
    stages = m.n_estimators_ if family == "gb" else m.n_iter_
    assert t.n_trees == stages * t.n_outputs
    if "single_node" in kind:
        assert t.n_nodes == t.n_trees  # every root is a leaf
    if "one_stage" in kind:
        assert t.n_trees == t.n_outputs
    x = np.random.default_rng(11).normal(size=(500, D)).astype(np.float32).astype(np.float64)
    got, want = t.decision_function_numpy(x), m.decision_function(x)
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)
    assert "single_node" in kind or np.unique(got).size > 2  # the trees tell rows apart
    # the float32 cast: a float32 copy of the rows gives the same bits
    np.testing.assert_array_equal(t.decision_function_numpy(x.astype(np.float32)), got)


@pytest.mark.parametrize("kind", list(KINDS))
def test_probabilities_within_ulps_of_sklearn(kind):
    m = _fit(kind)
    t = BoostTables.from_sklearn(m)
    x = np.random.default_rng(11).normal(size=(500, D)).astype(np.float32).astype(np.float64)
    got, want = t.predict_proba_numpy(x), m.predict_proba(x)
    assert got.shape == want.shape
    u = _ulps(got, want)
    print(f"{kind}: max ulps {u.max():.2f}, elements differing {int((got != want).sum())} of "
          f"{got.size}, max |diff| {np.abs(got - want).max():.3e}")
    assert u.max() <= MAX_ULP
    # K classes: the softmax's denominator carries K - 1 rounded additions, each quotient is
    # rounded once (together at most 2^-53 over a row, the p[k] summing to 1), and this check's
    # own sum rounds K - 1 times more: below 2 K half-ulps of 1
    np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=2 * got.shape[1] * 2.0 ** -53)


def test_det_exp_host_build():
    from moeva2_amd import _native

    x = np.array([0.0, -0.0, 1.0, -1.0, 40.0, -40.0, 709.78, 709.79, -745.13, -745.14, 800.0,
                  -800.0, np.inf, -np.inf, np.nan, -720.0])
    e = _native.det_exp(x)
    assert e[0] == 1.0 and e[1] == 1.0
    assert e[7] == np.inf and e[10] == np.inf and e[12] == np.inf
    assert e[9] == 0.0 and e[11] == 0.0 and e[13] == 0.0
    assert np.isnan(e[14])
    assert 0.0 < e[15] < np.finfo(np.float64).tiny  # a subnormal result
    fin = np.isfinite(e) & (e > np.finfo(np.float64).tiny)
    assert (_ulps(e[fin], np.exp(x[fin])) <= 1).all()
    r = np.random.default_rng(2).uniform(-700, 700, 20000)
    assert (_ulps(_native.det_exp(r), np.exp(r)) <= 1).all()


# A depth-1 tree on feature 0 and a root-only tree per stage: 2 stages, K = 2.
def _tables(**over):
    a = dict(n_features=3, n_classes=2, feature=[0, -1, -2, -3, 1, -4, -5, -6],
             threshold=[0.5, 0, 0, 0, -1.0, 0, 0, 0], left=[1, -1, -1, -1, 5, -1, -1, -1],
             right=[2, -1, -1, -1, 6, -1, -1, -1], tree_root=[0, 3, 4, 7],
             leaf_value=[1.0, -2.0, 0.25, 0.5, -0.5, 0.125], base=[-0.75])
    a.update(over)
    return a


def test_hand_written_tables():
    from moeva2_amd import _native

    t = BoostTables.from_arrays(**_tables())
    x = [[0.5, 0, 0], [np.nextafter(np.float32(0.5), 1), -1.0, 0], [np.nan, np.nan, 0]]
    raw = t.decision_function_numpy(x)
    np.testing.assert_array_equal(raw, [-0.75 + 1.0 + 0.25 - 0.5 + 0.125,
                                        -0.75 - 2.0 + 0.25 + 0.5 + 0.125,
                                        -0.75 - 2.0 + 0.25 - 0.5 + 0.125])
    p = t.predict_proba_numpy(x)
    p1 = 1.0 / (1.0 + _native.det_exp(-raw))
    np.testing.assert_array_equal(p, np.stack([1.0 - p1, p1], axis=1))
    # three classes, one stage of root-only trees: the softmax of base + leaf
    t3 = BoostTables.from_arrays(2, 3, [-1, -2, -3], [0, 0, 0], [-1] * 3, [-1] * 3, [0, 1, 2],
                                 [1.0, 2.0, -1.0], [0.5, 0.0, 0.25])
    np.testing.assert_array_equal(t3.decision_function_numpy([[0.0, 0.0]]), [[1.5, 2.0, -0.75]])
    p3 = t3.predict_proba_numpy([[0.0, 0.0]])[0]
    e = _native.det_exp(np.array([-0.5, 0.0, -2.75]))
    np.testing.assert_array_equal(p3, e / ((e[0] + e[1]) + e[2]))


BAD = {
    "child <= parent": dict(left=[0, -1, -1, -1, 5, -1, -1, -1]),
    "a child before its parent": dict(right=[2, -1, -1, -1, 3, -1, -1, -1]),
    "child outside its tree": dict(right=[3, -1, -1, -1, 6, -1, -1, -1]),
    "two parents": dict(right=[1, -1, -1, -1, 6, -1, -1, -1]),
    "feature >= D": dict(feature=[3, -1, -2, -3, 1, -4, -5, -6]),
    "1 class": dict(n_classes=1),
    "9 classes": dict(n_classes=9, base=[0.0] * 9),
    "0 trees": dict(tree_root=[]),
    "leaf index outside leaf_value": dict(feature=[0, -1, -2, -3, 1, -4, -5, -7]),
    "n_trees not a multiple of n_outputs": dict(n_classes=3, base=[0.0, 0.0, 0.0]),
    "two outputs for two classes": dict(base=[0.0, 0.0]),
    "one output for three classes": dict(n_classes=3),
    "base not finite": dict(base=[np.inf]),
    "leaf not finite": dict(leaf_value=[1.0, np.nan, 0.25, 0.5, -0.5, 0.125]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_table_checks_python(name):
    with pytest.raises(ValueError):
        BoostTables.from_arrays(**_tables(**BAD[name]))


def _raw_tables(a):
    return types.SimpleNamespace(n_features=a["n_features"], n_classes=a["n_classes"],
                                 feature=np.asarray(a["feature"], np.int32),
                                 threshold=np.asarray(a["threshold"], np.float64),
                                 left=np.asarray(a["left"], np.int32),
                                 right=np.asarray(a["right"], np.int32),
                                 tree_root=np.asarray(a["tree_root"], np.int32).reshape(-1),
                                 leaf_value=np.asarray(a["leaf_value"], np.float64),
                                 base=np.asarray(a["base"], np.float64))


@pytest.mark.parametrize("name", list(BAD))
def test_table_checks_c_abi(name):
    """mv_boost_create refuses the same tables with MV_ERR_ARG before any device call (so this
    runs without a GPU); the binding turns that into ValueError."""
    from moeva2_amd import _native

    with pytest.raises(ValueError):
        _native.Boost(_raw_tables(_tables(**BAD[name])))


def test_from_sklearn_refusals():
    from sklearn.ensemble import (GradientBoostingClassifier, HistGradientBoostingClassifier,
                                  RandomForestClassifier)
    from sklearn.linear_model import LogisticRegression

    X, y = _data(300, 2, 5)
    with pytest.raises(ValueError, match="loss"):
        BoostTables.from_sklearn(
            GradientBoostingClassifier(loss="exponential", n_estimators=3).fit(X, y))
    with pytest.raises(ValueError, match="init"):
        BoostTables.from_sklearn(
            GradientBoostingClassifier(init=LogisticRegression(), n_estimators=3).fit(X, y))
    Xc = X.copy()
    Xc[:, 0] = np.random.default_rng(1).integers(0, 4, X.shape[0])
    yc = (Xc[:, 0] % 2).astype(int)
    hc = HistGradientBoostingClassifier(max_iter=3, categorical_features=[0]).fit(Xc, yc)
    assert any(p.nodes["is_categorical"].any() for it in hc._predictors for p in it)
    with pytest.raises(ValueError, match="categorical"):
        BoostTables.from_sklearn(hc)
    X9, y9 = _data(900, 9, 6)
    for m in (GradientBoostingClassifier(n_estimators=1, max_depth=1),
              HistGradientBoostingClassifier(max_iter=1, max_depth=1)):
        with pytest.raises(ValueError, match="9 classes"):
            BoostTables.from_sklearn(m.fit(X9, y9))
    with pytest.raises(ValueError):
        BoostTables.from_sklearn(RandomForestClassifier(n_estimators=2).fit(X, y))


def test_npz_round_trip_and_load_model(tmp_path):
    import joblib

    from moeva2_amd.attacks.moeva2.classifier import load_model

    x = np.random.default_rng(3).normal(size=(40, D))
    for kind in ("gb3", "hist2"):
        m = _fit(kind)
        t = BoostTables.from_sklearn(m)
        path = t.save(str(tmp_path / kind))
        assert path.endswith(".npz")
        back = BoostTables.load(path)
        for k in ("feature", "threshold", "left", "right", "tree_root", "leaf_value", "base"):
            np.testing.assert_array_equal(getattr(back, k), getattr(t, k))
        assert (back.n_features, back.n_classes) == (t.n_features, t.n_classes)
        want = t.predict_proba_numpy(x)
        lm = load_model(path)
        assert isinstance(lm, BoostModel)
        np.testing.assert_array_equal(lm.boost_tables().predict_proba_numpy(x), want)
        jpath = str(tmp_path / (kind + ".joblib"))
        joblib.dump(m, jpath)
        lj = load_model(jpath)  # the parent commit raises ValueError here
        assert isinstance(lj, BoostModel)
        np.testing.assert_array_equal(lj.boost_tables().predict_proba_numpy(x), want)
    with pytest.raises(ValueError):
        BoostTables.load(_forest_file(tmp_path))


def _forest_file(tmp_path):
    from moeva2_amd.models.forest import ForestTables

    return ForestTables.from_arrays(1, [-1], [0.0], [-1], [-1], [0], [[0.5, 0.5]]).save(
        str(tmp_path / "forest"))


def test_device_classifier_detection():
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.problem import has_device_boost, has_device_classifier, has_device_forest

    gb = _fit("gb2")
    t = BoostTables.from_sklearn(gb)

    class OnlyProba:
        def predict_proba(self, x):
            return gb.predict_proba(x)

    for model, k in ((gb, 2), (_fit("hist3"), 3), (t, 2), (BoostModel(t), 2)):
        c = Classifier(model)
        assert has_device_classifier(c)  # False on the parent commit: the hosted path
        assert has_device_boost(c) and not has_device_forest(c)
        assert c.boost_tables().n_classes == k
        with pytest.raises(NotImplementedError):
            c.dense_weights()  # PGD and training keep refusing trees
        with pytest.raises(NotImplementedError):
            c.forest_tables()
    c = Classifier(OnlyProba())
    assert not has_device_classifier(c) and not has_device_boost(c)
    with pytest.raises(NotImplementedError):
        c.boost_tables()
    # a model outside the limits stays hosted
    from sklearn.ensemble import GradientBoostingClassifier

    X, y = _data(300, 2, 5)
    c = Classifier(GradientBoostingClassifier(loss="exponential", n_estimators=2).fit(X, y))
    assert not has_device_boost(c) and not has_device_classifier(c)


def test_exported_symbols_include_boost():
    from moeva2_amd import _native

    L = _native.lib()
    for s in ("mv_boost_create", "mv_engine_set_boost", "mv_det_exp"):
        assert s in _native.EXPORTED
        assert hasattr(L, s), f"{s} missing from the built library"


def test_boost_routes(tmp_path):
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("hipcc not found")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "moeva2-ijcai22-replication_amd", "csrc")
    exe = str(tmp_path / "boost_routes_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", csrc,
                    os.path.join(here, "native", "boost_routes_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    # a boosted ensemble -> BOOST_ROWS_LDS (10) while its packed nodes fit 64 KiB, else
    # BOOST_ROWS (9); zero boost fields -> the kinds test_routes_cpu.py / test_forest_cpu.py pin
    assert r.stdout.splitlines() == [
        "lcld boost 100 x depth 3 kind=10",
        "botnet boost 1 node      kind=10",
        "boost at the budget      kind=10",
        "boost one node over      kind=9",
        "boost 1.6 M nodes        kind=9",
        "lds switched off         kind=9",
        "forest, zero boost       kind=8",
        "no model, zero boost     kind=-1",
        "lcld 64-32-2, zero boost kind=7",
        "botnet 64-64-2, zero boost kind=6",
        "botnet hidden 256, zero boost kind=5",
        "lds switched off, zero boost kind=6",
        "FOREST_ROWS=8 BOOST_ROWS=9 BOOST_ROWS_LDS=10 budget_nodes=4096",
    ]
