"""Tree ensembles without a GPU: the restatement of scikit-learn's predict_proba
(moeva2_amd/models/forest.py), the table checks on the Python side and behind the C ABI (they
come before any device call), files, classifier detection, the exported symbols and the route.

Restatement vs sklearn 1.7.2: this sklearn version stores the leaf fractions in tree_.value
and no longer divides by their sum in predict_proba, so the restatement's ``value / sum``
differs from it in the last bit of some leaf rows (observed maximum 1.1e-16 on the forests
below: one ulp of a probability in [0.5, 1)).  The bound is therefore the 1e-15 absolute the
specification allows, not bit equality; stumps and single trees whose leaf sums are exactly 1
still agree to the bit, which the test also asserts.
"""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from moeva2_amd.models.forest import ForestModel, ForestTables

sklearn = pytest.importorskip("sklearn")


def _data(n, d, k, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    y = (np.abs(X[:, 0] * 3 + X[:, 1] * X[:, 2]) * 1.7).astype(int) % k
    return X, y


def _fit(kind):
    from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier

    if kind == "stump":
        m, k = RandomForestClassifier(n_estimators=1, max_depth=1, random_state=0), 2
    elif kind == "rf17":
        m, k = RandomForestClassifier(n_estimators=17, max_depth=12, random_state=1), 3
    elif kind == "extra":
        m, k = ExtraTreesClassifier(n_estimators=9, max_depth=8, random_state=2), 4
    elif kind == "rf8":
        m, k = RandomForestClassifier(n_estimators=5, max_depth=10, random_state=4), 8
    else:
        m, k = DecisionTreeClassifier(max_depth=9, random_state=3), 2
    X, y = _data(600, 11, k, 7)
    m.fit(X, y)
    return m


@pytest.mark.parametrize("kind", ["stump", "rf17", "extra", "tree", "rf8"])
def test_restatement_matches_sklearn(kind):
    m = _fit(kind)
    if hasattr(m, "n_jobs"):
        m.n_jobs = 1
    t = ForestTables.from_sklearn(m)
    assert t.n_trees == (len(m.estimators_) if hasattr(m, "estimators_") else 1)
    assert t.n_classes == m.n_classes_
    x = np.random.default_rng(11).normal(size=(500, 11))
    got, want = t.predict_proba_numpy(x), m.predict_proba(x)
    diff = np.abs(got - want).max()
    print(f"{kind}: max |restatement - sklearn| = {diff:.3e}, rows differing "
          f"{int((got != want).any(axis=1).sum())} of {x.shape[0]}")
    assert diff <= 1e-15
    if kind in ("stump", "tree"):
        np.testing.assert_array_equal(got, want)
    # the float32 cast is sklearn's: a float64 row that rounds across a threshold follows it
    np.testing.assert_array_equal(t.predict_proba_numpy(x.astype(np.float32)), got)


# A depth-1 tree on feature 0 and a root-only tree: 5 nodes, 3 leaves, 2 classes.
def _tables(**over):
    a = dict(n_features=3, feature=[0, -1, -2, -3], threshold=[0.5, 0, 0, 0],
             left=[1, -1, -1, -1], right=[2, -1, -1, -1], tree_root=[0, 3],
             leaf_value=[[1.0, 0.0], [0.25, 0.75], [0.5, 0.5]])
    a.update(over)
    return a


def test_hand_written_tables():
    t = ForestTables.from_arrays(**_tables())
    p = t.predict_proba_numpy([[0.5, 0, 0], [np.nextafter(np.float32(0.5), 1), 0, 0],
                               [np.nan, 0, 0]])
    np.testing.assert_array_equal(p, [[0.75, 0.25], [0.375, 0.625], [0.375, 0.625]])


BAD = {
    "child <= parent": dict(left=[0, -1, -1, -1]),
    "child == parent (right)": dict(right=[0, -1, -1, -1]),
    "child outside its tree": dict(right=[3, -1, -1, -1]),
    "child past the node array": dict(right=[9, -1, -1, -1]),
    "feature >= D": dict(feature=[3, -1, -2, -3]),
    "1 class": dict(leaf_value=[[1.0], [1.0], [1.0]]),
    "9 classes": dict(leaf_value=np.full((3, 9), 1 / 9)),
    "0 trees": dict(tree_root=[]),
    "leaf index outside leaf_value": dict(feature=[0, -1, -2, -4]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_table_checks_python(name):
    with pytest.raises(ValueError):
        ForestTables.from_arrays(**_tables(**BAD[name]))


@pytest.mark.parametrize("name", list(BAD))
def test_table_checks_c_abi(name):
    """mv_forest_create refuses the same tables with MV_ERR_ARG before any device call (so
    this runs without a GPU); the binding turns that into ValueError."""
    from moeva2_amd import _native

    a = _tables(**BAD[name])
    lv = np.asarray(a["leaf_value"], np.float64)
    raw = types.SimpleNamespace(n_features=a["n_features"], n_classes=lv.shape[1],
                                feature=np.asarray(a["feature"], np.int32),
                                threshold=np.asarray(a["threshold"], np.float64),
                                left=np.asarray(a["left"], np.int32),
                                right=np.asarray(a["right"], np.int32),
                                tree_root=np.asarray(a["tree_root"], np.int32).reshape(-1),
                                leaf_value=lv)
    with pytest.raises(ValueError):
        _native.Forest(raw)


def test_c_abi_refuses_a_node_with_two_parents():
    from moeva2_amd import _native

    # both children of the root are node 1: every index check passes, the walk is no tree
    raw = types.SimpleNamespace(n_features=1, n_classes=2, feature=np.array([0, -1, -2], np.int32),
                                threshold=np.zeros(3), left=np.array([1, -1, -1], np.int32),
                                right=np.array([1, -1, -1], np.int32),
                                tree_root=np.array([0], np.int32),
                                leaf_value=np.array([[1.0, 0.0], [0.0, 1.0]]))
    # ... and a node reached from its parent and from its grandparent
    chain = types.SimpleNamespace(**vars(raw))
    chain.feature = np.array([0, 0, -1, -2], np.int32)
    chain.threshold = np.zeros(4)
    chain.left = np.array([1, 2, -1, -1], np.int32)
    chain.right = np.array([2, 3, -1, -1], np.int32)
    for bad in (raw, chain):
        with pytest.raises(ValueError):
            _native.Forest(bad)


def test_npz_round_trip_and_load_model(tmp_path):
    import joblib

    from moeva2_amd.attacks.moeva2.classifier import load_model

    m = _fit("rf17")
    t = ForestTables.from_sklearn(m)
    path = t.save(str(tmp_path / "forest"))
    assert path.endswith(".npz")
    back = ForestTables.load(path)
    for k in ("feature", "threshold", "left", "right", "tree_root", "leaf_value"):
        np.testing.assert_array_equal(getattr(back, k), getattr(t, k))
    assert back.n_features == t.n_features
    x = np.random.default_rng(3).normal(size=(40, 11))
    want = t.predict_proba_numpy(x)
    lm = load_model(path)
    assert isinstance(lm, ForestModel)
    np.testing.assert_array_equal(lm.forest_tables().predict_proba_numpy(x), want)
    jpath = str(tmp_path / "forest.joblib")
    joblib.dump(m, jpath)
    lj = load_model(jpath)
    assert isinstance(lj, ForestModel)
    np.testing.assert_array_equal(lj.forest_tables().predict_proba_numpy(x), want)
    joblib.dump({"not": "a model"}, str(tmp_path / "other.joblib"))
    with pytest.raises(ValueError):
        load_model(str(tmp_path / "other.joblib"))


def test_device_classifier_detection():
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.problem import has_device_classifier, has_device_forest

    m = _fit("tree")
    t = ForestTables.from_sklearn(m)

    class OnlyProba:
        def predict_proba(self, x):
            return m.predict_proba(x)

    for model in (m, _fit("rf17"), t, ForestModel(t)):
        c = Classifier(model)
        assert has_device_classifier(c) and has_device_forest(c)
        assert c.forest_tables().n_classes == model_classes(model)
        with pytest.raises(NotImplementedError):
            c.dense_weights()  # PGD and training keep refusing it
    c = Classifier(OnlyProba())
    assert not has_device_classifier(c) and not has_device_forest(c)
    with pytest.raises(NotImplementedError):
        c.forest_tables()


def model_classes(model):
    if hasattr(model, "n_classes_"):
        return int(model.n_classes_)
    return model.forest_tables().n_classes


def test_exported_symbols_include_forest():
    from moeva2_amd import _native

    names = ("mv_forest_create", "mv_forest_destroy", "mv_forest_predict",
             "mv_engine_set_forest", "mv_objcalc_run_forest")
    L = _native.lib()
    for s in names:
        assert s in _native.EXPORTED
        assert hasattr(L, s), f"{s} missing from the built library"


def test_forest_route(tmp_path):
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("hipcc not found")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "moeva2-ijcai22-replication_amd", "csrc")
    exe = str(tmp_path / "forest_routes_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", csrc,
                    os.path.join(here, "native", "forest_routes_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    # trees -> FOREST_ROWS (8); zero trees -> the kinds tests/test_routes_cpu.py pins
    assert r.stdout.splitlines() == [
        "lcld forest 100 trees   kind=8",
        "botnet forest 1 tree    kind=8",
        "no model, zero trees    kind=-1",
        "lcld 64-32-2, zero trees kind=7",
        "botnet 64-64-2, zero trees kind=6",
        "botnet hidden 256, zero trees kind=5",
        "FOREST_ROWS=8",
    ]
