"""Kernel machines and logistic regression without a GPU: the restatement of scikit-learn's
predict_proba (moeva2_amd/models/svm.py), libsvm's coupling alone, the table checks on the
Python side and behind the C ABI (they come before any device call), files, classifier
detection, the exported symbols and the route.

Tolerance against sklearn.  The restatement sums in its own order with one fma per feature,
libsvm and BLAS in theirs, and its exp is the engine's (csrc/detmath.h), not the C library's.
Measured on the models and rows below with scikit-learn 1.7.2, maximum |difference| of a
probability: 2.2e-16 (svc_linear), 3.3e-16 (svc_poly), 7.8e-16 (svc_rbf), 3.3e-15 (nusvc_rbf,
whose decision values are the largest: they differ by 5.7e-14), 2.2e-16 / 1.1e-16 / 1.1e-16
(logistic regression, 2 / 3 / 8 classes).  The largest is MEASURED = 3.4e-15 (rounded up); the
bound is 8 times that for the summation-order difference on other data, fixed
before any device run.
"""
import os
import shutil
import subprocess
import types
import warnings

import numpy as np
import pytest

from moeva2_amd.models.svm import SvmModel, SvmTables, couple2, powi

sklearn = pytest.importorskip("sklearn")

MEASURED = 3.4e-15
TOL = 8 * MEASURED
D = 11


def _data(n, k, seed):
    """float32-representable rows, a label that depends on several features."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D)).astype(np.float32).astype(np.float64)
    y = (np.abs(X[:, 0] * 3 + X[:, 1] * X[:, 2]) * 1.7).astype(int) % k
    return X, y


def _make(kind):
    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import SVC, NuSVC

    X, y = _data(300, 2, 7)
    if kind == "svc_linear":
        return SVC(kernel="linear", probability=True, random_state=0).fit(X, y)
    if kind == "svc_poly":
        return SVC(kernel="poly", degree=3, coef0=1, probability=True, random_state=0).fit(X, y)
    if kind == "svc_rbf":
        return SVC(kernel="rbf", probability=True, random_state=0).fit(X, y)
    if kind == "nusvc_rbf":
        return NuSVC(kernel="rbf", probability=True, random_state=0).fit(X, y)
    if kind == "svc_labels_3_7":
        return SVC(kernel="rbf", probability=True, random_state=0).fit(X, np.where(y == 0, 7, 3))
    k = {"lr2": 2, "lr3": 3, "lr8": 8}[kind]
    return LogisticRegression().fit(*_data(300, k, 7))


KINDS = ("svc_linear", "svc_poly", "svc_rbf", "nusvc_rbf", "lr2", "lr3", "lr8")
_FITTED = {}


def _fit(kind):
    if kind not in _FITTED:
        _FITTED[kind] = _make(kind)
    return _FITTED[kind]


def _rows():
    return _data(500, 2, 11)[0]


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_against_sklearn(kind):
    m = _fit(kind)
    t = SvmTables.from_sklearn(m)
    assert t.n_features == D and t.n_classes == len(m.classes_)
    if kind.startswith("lr"):
        assert t.coef is None and t.kernel == "linear" and t.n_vec == t.n_out
        assert t.link == ("sigmoid" if t.n_classes == 2 else "softmax")
    else:
        assert t.link == "platt" and t.n_out == 1 and t.coef.shape == (1, t.n_vec)
        assert t.n_vec == m.support_vectors_.shape[0] and t.gamma == m._gamma
    x = _rows()
    got, want = t.predict_proba_numpy(x), m.predict_proba(x)
    assert got.shape == want.shape and got.dtype == want.dtype
    dec = np.abs(t.decision_function_numpy(x) - m.decision_function(x)).max()
    diff = np.abs(got - want).max()
    print(f"{kind}: n_vec {t.n_vec}, max |decision diff| {dec:.3e}, max |proba diff| {diff:.3e}")
    assert diff <= TOL
    assert np.unique(got[:, 0]).size > 100  # the model tells the rows apart
    # the float32 cast: a float32 copy of the rows gives the same bits
    np.testing.assert_array_equal(t.predict_proba_numpy(x.astype(np.float32)), got)
    # the order of every sum is fixed: one row alone gives the bits it has in the batch
    np.testing.assert_array_equal(t.predict_proba_numpy(x[7:8]), got[7:8])


def test_class_column_order():
    m = _fit("svc_labels_3_7")
    assert list(m.classes_) == [3, 7]
    t = SvmTables.from_sklearn(m)
    x = _rows()
    got, want = t.predict_proba_numpy(x), m.predict_proba(x)
    assert np.abs(got - want).max() <= TOL
    # the columns are far apart (against the bound) on most rows: a swap could not pass it
    assert (np.abs(want[:, 0] - want[:, 1]) > 1e-3).mean() > 0.9
    assert np.abs(got[:, ::-1] - want).max() > 1e-3


def test_powi_is_libsvm_s():
    b = np.array([1.5, -2.25, 0.0, 3.0])
    np.testing.assert_array_equal(powi(b, 0), np.ones(4))
    np.testing.assert_array_equal(powi(b, 1), b)
    np.testing.assert_array_equal(powi(b, 3), b * (b * b))
    np.testing.assert_array_equal(powi(b, 5), b * ((b * b) * (b * b)))


def test_coupling_alone():
    """libsvm's multiclass_probability for two classes at the clip edges and at 0.5."""
    r = np.array([1e-7, 1 - 1e-7, 0.5, 0.25, 0.9])
    p, it = couple2(r, return_iters=True)
    assert p.shape == (5, 2)
    assert (it < 100).all() and it[2] == 0  # (0.5, 0.5) is already the fixed point
    np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(p[2], [0.5, 0.5])
    assert (p >= 0).all() and (p <= 1).all()
    assert p[0, 0] < 0.5 < p[1, 0] and p[3, 0] < 0.5 < p[4, 0]
    # a NaN ends the loop at its first test: the start point, no NaN written
    pn, itn = couple2(np.array([np.nan]), return_iters=True)
    assert itn[0] == 0
    np.testing.assert_array_equal(pn[0], [0.5, 0.5])
    # elementwise: a batch gives each element the bits it has alone
    for i in range(r.size):
        np.testing.assert_array_equal(couple2(r[i:i + 1])[0], p[i])


def test_svm_sums_host_build():
    """mv_svm_sums is a chain of fused multiply-adds in ascending feature order."""
    from moeva2_amd import _native

    e = 2.0 ** -30
    x = np.array([[-(1 + 2 * e), 1 + e, 0.0], [3.0, 4.0, 5.0]])
    v = np.array([[1.0, 1 + e, 7.0], [0.5, 0.25, 2.0]])
    s = _native.svm_sums(x, v, False)
    # row 0, vector 0: fma(1 + e, 1 + e, -(1 + 2 e)) = e^2, which a rounded product loses
    assert s[0, 0] == e * e and x[0, 0] * v[0, 0] + x[0, 1] * v[0, 1] == 0.0
    assert s[1, 1] == 3 * 0.5 + 4 * 0.25 + 5 * 2.0
    r = _native.svm_sums(x, v, True)
    assert r[1, 1] == 2.5 ** 2 + 3.75 ** 2 + 3.0 ** 2
    np.testing.assert_allclose(r, ((x[:, None, :] - v[None]) ** 2).sum(-1), rtol=1e-15)
    with pytest.raises(ValueError):
        _native.svm_sums(x, v[:, :2], False)


# ---------------------------------------------------------------- table checks
def _tables(**over):
    a = dict(n_features=3, n_classes=2, vectors=[[0.5, -1.0, 2.0], [1.0, 0.25, -0.5]],
             coef=[[1.5, -0.75]], intercept=[0.125], kernel="rbf", gamma=0.5, coef0=0.0,
             degree=3, link="platt", probA=-1.25, probB=0.1)
    a.update(over)
    return a


BAD = {
    "kernel sigmoid": dict(kernel="sigmoid"),
    "kernel precomputed": dict(kernel="precomputed"),
    "kernel callable": dict(kernel=lambda a, b: a @ b.T),
    "degree 2.5": dict(kernel="poly", degree=2.5),
    "degree -1": dict(kernel="poly", degree=-1),
    "degree 65": dict(kernel="poly", degree=65),
    "platt with 3 classes": dict(n_classes=3),
    "softmax with 2 classes": dict(link="softmax"),
    "softmax with one decision": dict(link="softmax", n_classes=3),
    "9 classes": dict(link="softmax", n_classes=9, coef=None, intercept=[0.0] * 9,
                      vectors=np.ones((9, 3)), kernel="linear"),
    "1 class": dict(n_classes=1),
    "no vector": dict(vectors=np.zeros((0, 3)), coef=np.zeros((1, 0))),
    "coef of another shape": dict(coef=[[1.0, 2.0, 3.0]]),
    "identity with n_vec != n_out": dict(coef=None, link="sigmoid", kernel="linear"),
    "vector not finite": dict(vectors=[[0.5, np.nan, 2.0], [1.0, 0.25, -0.5]]),
    "coef not finite": dict(coef=[[np.inf, 1.0]]),
    "intercept not finite": dict(intercept=[np.nan]),
    "gamma not finite": dict(gamma=np.inf),
    "probA not finite": dict(probA=np.nan),
    "n_vec * D above the limit": dict(n_features=4096, vectors=np.zeros((4097, 4096)),
                                      coef=np.zeros((1, 4097))),
}


def test_valid_tables_pass():
    t = SvmTables.from_arrays(**_tables())
    assert (t.n_vec, t.n_out, t.n_classes) == (2, 1, 2)
    p = t.predict_proba_numpy([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]])
    assert p.shape == (3, 2) and np.isfinite(p).all()  # the clip takes a NaN to 1e-7
    # at the limit exactly
    SvmTables.from_arrays(**_tables(n_features=4096, vectors=np.zeros((4096, 4096)),
                                    coef=np.zeros((1, 4096))))


@pytest.mark.parametrize("name", list(BAD))
def test_table_checks_python(name):
    with pytest.raises(ValueError):
        SvmTables.from_arrays(**_tables(**BAD[name]))


def _raw_tables(a):
    return types.SimpleNamespace(
        n_features=a["n_features"], n_classes=a["n_classes"],
        vectors=np.asarray(a["vectors"], np.float64),
        coef=None if a["coef"] is None else np.asarray(a["coef"], np.float64),
        intercept=np.asarray(a["intercept"], np.float64), kernel=a["kernel"], gamma=a["gamma"],
        coef0=a["coef0"], degree=a["degree"], link=a["link"], probA=a["probA"], probB=a["probB"])


@pytest.mark.parametrize("name", list(BAD))
def test_table_checks_c_abi(name):
    """_native.Svm refuses the same tables before any device call (so this runs without a GPU):
    the binding for what mv_svm_desc cannot express (a kernel's name, a fractional degree, a
    coef of another shape), mv_svm_create with MV_ERR_ARG for the rest; both are ValueError."""
    from moeva2_amd import _native

    with pytest.raises(ValueError):
        _native.Svm(_raw_tables(_tables(**BAD[name])))


def test_from_sklearn_refusals():
    import scipy.sparse as sps
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import SVC, LinearSVC

    X, y = _data(120, 2, 5)
    X3, y3 = _data(150, 3, 5)
    with pytest.raises(ValueError, match="kernel"):
        SvmTables.from_sklearn(SVC(kernel="sigmoid", probability=True).fit(X, y))
    with pytest.raises(ValueError, match="kernel"):
        SvmTables.from_sklearn(SVC(kernel="precomputed", probability=True).fit(X @ X.T, y))
    with pytest.raises(ValueError, match="kernel"):
        SvmTables.from_sklearn(SVC(kernel=lambda a, b: a @ b.T, probability=True).fit(X, y))
    with pytest.raises(ValueError, match="probability"):
        SvmTables.from_sklearn(SVC(kernel="rbf").fit(X, y))
    with pytest.raises(ValueError, match="3 classes"):
        SvmTables.from_sklearn(SVC(kernel="rbf", probability=True).fit(X3, y3))
    with pytest.raises(ValueError, match="sparse"):
        SvmTables.from_sklearn(SVC(kernel="rbf", probability=True).fit(sps.csr_matrix(X), y))
    with pytest.raises(ValueError, match="degree"):
        SvmTables.from_sklearn(SVC(kernel="poly", degree=2.5, probability=True).fit(X, y))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ovr = LogisticRegression(multi_class="ovr").fit(X3, y3)
        mn2 = LogisticRegression(multi_class="multinomial").fit(X, y)
    with pytest.raises(ValueError, match="one-vs-rest"):
        SvmTables.from_sklearn(ovr)
    with pytest.raises(ValueError, match="multinomial"):
        SvmTables.from_sklearn(mn2)
    with pytest.raises(ValueError, match="9 classes"):
        SvmTables.from_sklearn(LogisticRegression().fit(*_data(400, 9, 6)))
    for other in (LinearSVC().fit(X, y), RandomForestClassifier(n_estimators=2).fit(X, y)):
        with pytest.raises(ValueError):
            SvmTables.from_sklearn(other)


def test_npz_round_trip_and_load_model(tmp_path):
    import joblib

    from moeva2_amd.attacks.moeva2.classifier import load_model

    x = np.random.default_rng(3).normal(size=(40, D))
    for kind in ("svc_poly", "nusvc_rbf", "lr2", "lr3"):
        m = _fit(kind)
        t = SvmTables.from_sklearn(m)
        path = t.save(str(tmp_path / kind))
        assert path.endswith(".npz")
        back = SvmTables.load(path)
        for k in ("vectors", "intercept"):
            np.testing.assert_array_equal(getattr(back, k), getattr(t, k))
        if t.coef is None:
            assert back.coef is None
        else:
            np.testing.assert_array_equal(back.coef, t.coef)
        for k in ("n_features", "n_classes", "kernel", "link", "degree", "gamma", "coef0", "probA",
                  "probB"):
            assert getattr(back, k) == getattr(t, k), k
        want = t.predict_proba_numpy(x)
        lm = load_model(path)
        assert isinstance(lm, SvmModel)
        np.testing.assert_array_equal(lm.svm_tables().predict_proba_numpy(x), want)
        jpath = str(tmp_path / (kind + ".joblib"))
        joblib.dump(m, jpath)
        lj = load_model(jpath)  # the parent commit raises ValueError here
        assert isinstance(lj, SvmModel)
        np.testing.assert_array_equal(lj.svm_tables().predict_proba_numpy(x), want)
    dpath = str(tmp_path / "dict.joblib")
    joblib.dump({"not": "a model"}, dpath)
    with pytest.raises(ValueError):
        load_model(dpath)
    from moeva2_amd.models.forest import ForestTables

    fpath = ForestTables.from_arrays(1, [-1], [0.0], [-1], [-1], [0], [[0.5, 0.5]]).save(
        str(tmp_path / "forest"))
    with pytest.raises(ValueError):
        SvmTables.load(fpath)


def test_device_classifier_detection():
    from sklearn.svm import SVC

    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.problem import (has_device_boost, has_device_classifier, has_device_forest,
                                    has_device_svm)

    svc = _fit("svc_rbf")
    t = SvmTables.from_sklearn(svc)

    class OnlyProba:
        def predict_proba(self, x):
            return svc.predict_proba(x)

    for model, k in ((svc, 2), (_fit("nusvc_rbf"), 2), (_fit("lr8"), 8), (t, 2), (SvmModel(t), 2)):
        c = Classifier(model)
        assert has_device_classifier(c)  # False on the parent commit: the hosted path
        assert has_device_svm(c) and not has_device_forest(c) and not has_device_boost(c)
        assert c.svm_tables().n_classes == k
        for refused in (c.dense_weights, c.forest_tables, c.boost_tables):
            with pytest.raises(NotImplementedError):
                refused()  # PGD and training keep refusing these models
    c = Classifier(OnlyProba())
    assert not has_device_classifier(c) and not has_device_svm(c)
    with pytest.raises(NotImplementedError):
        c.svm_tables()
    # a model outside the limits stays hosted
    X, y = _data(120, 2, 5)
    c = Classifier(SVC(kernel="sigmoid", probability=True).fit(X, y))
    assert not has_device_svm(c) and not has_device_classifier(c)


def test_exported_symbols_include_svm():
    from moeva2_amd import _native

    L = _native.lib()
    for s in ("mv_svm_create", "mv_engine_set_svm", "mv_svm_sums"):
        assert s in _native.EXPORTED
        assert hasattr(L, s), f"{s} missing from the built library"


def test_svm_routes(tmp_path):
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("hipcc not found")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "moeva2-ijcai22-replication_amd", "csrc")
    exe = str(tmp_path / "svm_routes_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", csrc,
                    os.path.join(here, "native", "svm_routes_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    # svm fields set -> SVM_ROWS (11) at any size; zero svm fields -> the kinds
    # test_routes_cpu.py / test_forest_cpu.py / test_boost_cpu.py pin
    assert r.stdout.splitlines() == [
        "lcld svc 182 vectors     kind=11",
        "botnet logreg 1 vector   kind=11",
        "lcld svc 22000 vectors   kind=11",
        "forest, zero svm         kind=8",
        "boost, zero svm          kind=10",
        "no model, zero svm       kind=-1",
        "lcld 64-32-2, zero svm   kind=7",
        "botnet 64-64-2, zero svm kind=6",
        "botnet hidden 256, zero svm kind=5",
        "SVM_ROWS=11 SVM_VB=16 SVM_FC=16",
    ]
