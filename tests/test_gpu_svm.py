"""Kernel machines and logistic regression on the device (csrc/svm.hip k_svm) against the
restatement of scikit-learn's predict_proba (moeva2_amd/models/svm.py predict_proba_numpy).

There is no tolerance on a probability or on f1: the device performs the restatement's fp64
operations in its order (the feature sums through the host build of the same inline function,
the exp through csrc/detmath.h's), so any difference is a bug.  The shapes sit on the kernel's
tile edges: SVM_VB = 16 vectors per block, SVM_FC = 16 features per chunk, 64 rows per
workgroup.  The attack tests hold the device loop against the hosted loop (the same tables'
restatement behind a predict_proba-only wrapper): with bit-equal f1 both loops give the same
populations."""
import numpy as np
import pytest

import synth_problem as sp
from oracle import device_order as do
from test_gpu_forest import Lcld, eval_rows, ml_rows

from moeva2_amd.models.svm import SvmModel, SvmTables

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SVM_ROWS = 11
VB, FC = 16, 16  # csrc/svm.h SVM_VB, SVM_FC
ROWS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class OnlyProba:
    """The same tables as a model the engine cannot compile: the hosted loop."""

    def __init__(self, tables):
        self.tables = tables

    def predict_proba(self, x):
        return self.tables.predict_proba_numpy(x)


# ---------------------------------------------------------------- tables
def random_tables(rng, kind, n_vec, d, center=None, spread=1.0):
    """Hand-built tables of one kernel and link.  kind:
      linear / poly1 / poly5 / rbf   Platt's sigmoid and the coupling (an SVC)
      rbf_sigmoid                    coef [1][n_vec] and the plain sigmoid
      poly3_softmax3                 coef [3][n_vec] and the softmax
      lr2 / lr3 / lr8                no coef: the vectors are the decisions' rows (n_vec = K)"""
    c = np.zeros(d) if center is None else center
    vec = c + spread * rng.normal(size=(n_vec, d))
    a = 1.5 / np.sqrt(n_vec)
    if kind.startswith("lr"):
        k = int(kind[2:])
        assert n_vec == (1 if k == 2 else k)
        return SvmTables.from_arrays(d, k, vec / np.sqrt(d), None, rng.normal(size=n_vec) * 0.3,
                                     "linear", link="sigmoid" if k == 2 else "softmax")
    if kind == "rbf_sigmoid":
        return SvmTables.from_arrays(d, 2, vec, a * rng.normal(size=(1, n_vec)), [0.1], "rbf",
                                     gamma=0.7 / d, link="sigmoid")
    if kind == "poly3_softmax3":
        return SvmTables.from_arrays(d, 3, vec, a * rng.normal(size=(3, n_vec)),
                                     rng.normal(size=3) * 0.2, "poly", gamma=0.5 / d, coef0=0.5,
                                     degree=3, link="softmax")
    kernel = {"linear": "linear", "poly1": "poly", "poly5": "poly", "rbf": "rbf"}[kind]
    degree = {"poly1": 1, "poly5": 5}.get(kind, 3)
    return SvmTables.from_arrays(d, 2, vec, a * rng.normal(size=(1, n_vec)), [-0.2], kernel,
                                 gamma=0.6 / d, coef0=1.0, degree=degree, link="platt",
                                 probA=-1.7, probB=0.15)


SVC_KINDS = ("linear", "poly1", "poly5", "rbf", "rbf_sigmoid", "poly3_softmax3")


def check_predict(t, rng, what):
    """mv_forest_predict on an svm handle, every row count, into NaN-preset outputs; one row
    holds a NaN, one +inf and one -inf (defined behaviour: compared with equal NaNs)."""
    from moeva2_amd import _native

    f = _native.Svm(t)
    assert isinstance(f, _native.Forest)  # the forest handle
    d, nc = t.n_features, t.n_classes
    seen = []
    for n in ROWS:
        x = rng.normal(size=(n, d))
        if n >= 63:
            x[1, 0] = np.nan
            x[2, d - 1] = np.inf
            x[3, d // 2] = -np.inf
            x[4] = 1e30  # float32-representable, its square is not: rbf's sum stays finite in fp64
        xd = torch.as_tensor(x, device="cuda")
        out = torch.full((n + 1, nc), float("nan"), dtype=torch.float64, device="cuda")
        f.predict(xd, out[:n])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isnan(got[n]).all(), f"{what}, {n} rows: a write past the last row"
        want = t.predict_proba_numpy(x)
        np.testing.assert_array_equal(got[:n], want, err_msg=f"{what}, {n} rows")
        seen.append(want[5:] if n >= 63 else want)
    seen = np.concatenate(seen)
    assert np.isfinite(seen).all() and np.unique(seen[:, 0]).size > seen.shape[0] // 4, \
        f"{what}: the model does not tell the rows apart"


@pytest.mark.parametrize("d", [1, 3, 11, FC + 1])
@pytest.mark.parametrize("n_vec", [1, VB - 1, VB, VB + 1])
def test_svm_predict_bit_exact(n_vec, d):
    rng = np.random.default_rng(100 * n_vec + d)
    for kind in SVC_KINDS:
        check_predict(random_tables(rng, kind, n_vec, d), rng, f"{kind}, n_vec {n_vec}, D {d}")


@pytest.mark.parametrize("d", [1, 3, 11, FC + 1, 2 * FC, 3 * FC + 5])
def test_logistic_regression_predict_bit_exact(d):
    rng = np.random.default_rng(7 + d)
    for kind in ("lr2", "lr3", "lr8"):
        k = int(kind[2:])
        check_predict(random_tables(rng, kind, 1 if k == 2 else k, d), rng, f"{kind}, D {d}")


def test_saturating_links_bit_exact():
    """Decisions of +-40 and +-800: Platt's sigmoid reaches its clip on both sides (and the
    coupling runs from there), the plain sigmoid and the softmax reach 0 and 1."""
    rng = np.random.default_rng(2)
    for link, nc in (("platt", 2), ("sigmoid", 2), ("softmax", 3)):
        no = 1 if nc == 2 else nc
        coef = np.zeros((no, 2))
        coef[0] = [40.0, 800.0]
        if no > 1:
            coef[1] = [-40.0, 1.0]
        t = SvmTables.from_arrays(2, nc, np.eye(2), coef, np.zeros(no), "linear", link=link,
                                  probA=-1.0, probB=0.0)
        from moeva2_amd import _native

        x = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [0.0, 0.0], [0.5, 0.25]])
        x = np.concatenate([x, rng.normal(size=(70, 2))])
        out = torch.empty((x.shape[0], nc), dtype=torch.float64, device="cuda")
        _native.Svm(t).predict(torch.as_tensor(x, device="cuda"), out)
        torch.cuda.synchronize()
        want = t.predict_proba_numpy(x)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=link)
        if link == "platt":
            assert want[:4].min() < 1e-6 and want[:4].max() > 1 - 1e-6
        else:
            assert 0.0 in want[:4] and 1.0 in want[:4]


def test_fitted_models_predict_on_the_device():
    """SvmModel.predict_proba (the device) on fitted scikit-learn models: the restatement's bits."""
    from sklearn.linear_model import LogisticRegression
    from sklearn.svm import SVC, NuSVC

    rng = np.random.default_rng(3)
    X = rng.normal(size=(300, 11)).astype(np.float32).astype(np.float64)
    y = (np.abs(X[:, 0] * 3 + X[:, 1] * X[:, 2]) * 1.7).astype(int)
    x = rng.normal(size=(130, 11))
    for m in (SVC(kernel="rbf", probability=True, random_state=0).fit(X, y % 2),
              NuSVC(kernel="poly", degree=3, coef0=1, probability=True, random_state=0).fit(X, y % 2),
              LogisticRegression().fit(X, y % 2), LogisticRegression().fit(X, y % 3)):
        t = SvmTables.from_sklearn(m)
        np.testing.assert_array_equal(SvmModel(t).predict_proba(x), t.predict_proba_numpy(x),
                                      err_msg=type(m).__name__)


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("svm_synth")
    cache = {}

    def get(name):
        if name not in cache:
            sy = Lcld() if name == "lcld" else sp.build(name, d)
            if name != "lcld":
                sy.name = name
            sy.svm = {}
            cache[name] = sy
        return cache[name]

    return get


def calibrated(t, x):
    """t with its gamma (poly), its coefficients (or, without coef, its vectors) and its
    intercepts reset so that the decisions over the rows x straddle 0 and spread over a few
    units: no link saturates on them."""
    from moeva2_amd import _native

    x32 = np.asarray(x, np.float32).astype(np.float64)
    gamma = t.gamma
    if t.kernel == "poly":
        gamma = 0.6 / np.abs(_native.svm_sums(x32, t.vectors, False)).max()

    def build(vectors, coef, intercept):
        return SvmTables.from_arrays(t.n_features, t.n_classes, vectors, coef, intercept,
                                     t.kernel, gamma, t.coef0, t.degree, t.link, t.probA, t.probB)

    zero = np.zeros_like(t.intercept)
    dec = build(t.vectors, t.coef, zero).decision_function_numpy(x).reshape(x.shape[0], -1)
    k = 1.5 / max(float(dec.std(axis=0).max()), 1e-300)
    icpt = t.intercept - k * dec.mean(axis=0)  # centred: the decisions straddle 0
    if t.coef is None:
        return build(t.vectors * k, None, icpt)
    return build(t.vectors, t.coef * k, icpt)


def case_svm(sy, kind):
    """Tables over every feature of the problem (mutable ones come from the fp32 ML row, the
    others from xfix), the vectors spread around the ML rows the test evaluates."""
    if kind in sy.svm:
        return sy.svm[kind]
    genes = eval_rows(sy)
    x = np.concatenate([ml_rows(sy, b, genes[b]) for b in range(sp.B)])
    rng = np.random.default_rng(41)
    n_vec = {"lr2": 1, "lr3": 3}.get(kind, 2 * VB + 5)
    t = calibrated(random_tables(rng, kind, n_vec, x.shape[1], center=x.mean(axis=0),
                                 spread=x.std(axis=0) + 0.05), x)
    sy.svm[kind] = t
    return t


def svm_engine(sy, tables, mc=1):
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.problem import get_engine

    eng = get_engine(sy.constraints, Classifier(tables), sy.scaler, 2)
    xl, xu = sy.bounds()
    eng.set_states(sy.X, xl, xu, mc)
    return eng


@pytest.mark.parametrize("kind", ["rbf", "poly5", "linear", "lr2", "lr3", "poly3_softmax3"])
@pytest.mark.parametrize("name", ["lcld", "n8p", "c129"])
def test_evaluate_f1_bit_exact(cases, name, kind):
    """mv_evaluate's F[..][0] for 3 states x 37 rows: features the attack moves (the fp32 ML
    row) and features it does not (xfix), a minimize_class of each class."""
    sy = cases(name)
    t = case_svm(sy, kind)
    top = t.n_classes - 1
    for mc in (np.array([top, 0, top // 2 + top % 2]), np.array([0, top, 0])):
        eng = svm_engine(sy, t, mc=mc)
        assert eng.mlp_kernel() == SVM_ROWS
        assert eng.stored_genes().all()  # the full gene layout, as with a forest
        genes = eval_rows(sy)
        n = genes.shape[1]
        F = torch.full((sp.B, n, 3), float("nan"), dtype=torch.float64, device="cuda")
        eng.evaluate(torch.as_tensor(genes, device="cuda"), F)
        torch.cuda.synchronize()
        F = F.cpu().numpy()
        for b, prob in enumerate(sy.probs):
            what = f"{name}, {kind}, state {b}, class {mc[b]}"
            want = t.predict_proba_numpy(ml_rows(sy, b, genes[b]))[:, mc[b]]
            np.testing.assert_array_equal(F[b, :, 0], want, err_msg=what)
            ref = do.evaluate_device_order(prob, genes[b], sy.codes)
            np.testing.assert_array_equal(F[b, :, 1], ref[:, 1], err_msg=what)
        assert np.unique(F[:, :, 0]).size > 3, "the model does not tell these rows apart"


def attack(sy, model, mc, seed=7, streams=False, X=None, first_state=0, crossover="two_point",
           history="full"):
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2

    m = Moeva2(model, sy.constraints, ml_scaler=sy.scaler, norm=2, n_gen=4, n_pop=37,
               n_offsprings=20, save_history=history, seed=seed, state_streams=streams,
               crossover=crossover)
    X = sy.X if X is None else X
    out = m.generate(X, mc, return_device=True, first_state=first_state)
    torch.cuda.synchronize()
    return (m,) + tuple(None if o is None else o.cpu().numpy() for o in out)


@pytest.mark.parametrize("crossover,history,kind,mc",
                         [("two_point", "full", "rbf", 1), ("sbx", None, "poly5", (1, 0, 1)),
                          ("two_point", None, "lr3", (2, 0, 1))],
                         ids=["two_point_history_rbf", "sbx_poly5", "two_point_lr3"])
def test_attack_device_loop_equals_hosted_loop(cases, crossover, history, kind, mc):
    """Moeva2.generate with an SvmModel, 3 states, 4 generations: the device loop (offspring f1
    written through out_map, the history's f1 column) against the hosted loop driven by the
    restatement: f1 is bit-equal, so the trajectories are identical."""
    sy = cases("lcld")
    t = case_svm(sy, kind)
    mc = np.asarray(mc) if isinstance(mc, tuple) else mc
    md, gd, Fd, hd = attack(sy, SvmModel(t), mc, crossover=crossover, history=history)
    assert md.last_engine.mlp_kernel() == SVM_ROWS
    mh, gh, Fh, hh = attack(sy, OnlyProba(t), mc, crossover=crossover, history=history)
    assert mh.last_engine.mlp_kernel() == -1  # the hosted loop
    if history:
        assert hd.shape == (sp.B, 40 + 3 * 20, 3 + md.last_engine.prog.C)
        np.testing.assert_array_equal(hd, hh)
        assert np.unique(hd[:, :, 0]).size > 3
    else:
        assert hd is None and hh is None
    np.testing.assert_array_equal(gd, gh)
    np.testing.assert_array_equal(Fd, Fh)
    assert (gd != gd[:, :1]).any()
    # the final f1 is the restatement of the decoded final population
    for b in range(sp.B):
        want = t.predict_proba_numpy(ml_rows(sy, b, gd[b]))[:, np.broadcast_to(mc, sp.B)[b]]
        np.testing.assert_array_equal(Fd[b, :, 0], want)


def test_state_streams_state_equals_its_own_run(cases):
    sy = cases("lcld")
    t = case_svm(sy, "rbf")
    _, g3, F3, h3 = attack(sy, t, 1, streams=True)
    for b in range(sp.B):
        _, g1, F1, h1 = attack(sy, t, 1, streams=True, X=sy.X[b:b + 1], first_state=b)
        np.testing.assert_array_equal(g1[0], g3[b])
        np.testing.assert_array_equal(F1[0], F3[b])
        np.testing.assert_array_equal(h1[0], h3[b])
    assert (g3[0] != g3[1]).any()


def test_objective_calculator_device_equals_numpy(cases):
    """ObjectiveCalculator with an SvmModel (the device scoring path) equals the host
    computation through the restatement."""
    from moeva2_amd.attacks.moeva2.classifier import Classifier
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator

    sy = cases("lcld")
    t = case_svm(sy, "rbf")
    m, g, _, _ = attack(sy, t, 1, history=None)
    x_f = np.stack([m._encoder.genetic_to_ml(g[b], sy.X[b]) for b in range(sp.B)])
    thr = {"f1": 0.5, "f2": 4.0}
    dev = ObjectiveCalculator(Classifier(SvmModel(t)), sy.constraints, 1, thr,
                              min_max_scaler=sy.scaler, ml_scaler=sy.scaler, norm=2)
    host = ObjectiveCalculator(Classifier(OnlyProba(t)), sy.constraints, 1, thr,
                               min_max_scaler=sy.scaler, ml_scaler=sy.scaler, norm=2)
    assert type(dev._device()[2]).__name__ == "Svm" and host._device()[2] is None
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


def test_set_svm_preconditions(cases):
    """mv_engine_set_svm on an engine that has a model, after mv_set_states, a second time or
    with a wrong D returns the documented error (3 = MV_ERR_STATE, ValueError for MV_ERR_ARG),
    as the forest and boost tests assert them."""
    from moeva2_amd import _native
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.io.tf_bundle import DenseMLP
    from moeva2_amd.problem import get_engine

    sy = cases("n8p")
    t = case_svm(sy, "rbf")
    mlp = Classifier(DenseMLPModel(DenseMLP(sy.W, sy.bs, ["relu", "relu", "softmax"])))
    eng = get_engine(sy.constraints, mlp, sy.scaler, 2)
    with pytest.raises(_native.NativeError, match="error 3"):
        eng.set_svm(t)
    assert eng.forest is None and eng.mlp_kernel() != SVM_ROWS
    hosted = get_engine(sy.constraints, Classifier(OnlyProba(t)), sy.scaler, 2)
    xl, xu = sy.bounds()
    hosted.set_states(sy.X, xl, xu, 1)
    with pytest.raises(_native.NativeError, match="error 3"):
        hosted.set_svm(t)
    assert hosted.mlp_kernel() == -1
    with pytest.raises(_native.NativeError, match="error 3"):
        svm_engine(sy, t).set_svm(t)
    other = SvmTables.from_arrays(t.n_features + 1, 2, np.ones((1, t.n_features + 1)), [[1.0]],
                                  [0.0], "linear", link="sigmoid")
    fresh = _native.Engine(hosted.prog, None, None)
    with pytest.raises(ValueError):
        fresh.set_svm(other)
    assert fresh.mlp_kernel() == -1
    # minimize_class outside the model's classes
    with pytest.raises(_native.NativeError):
        svm_engine(sy, t, mc=2)
    # the bf16 mode is the Dense MLP's
    with pytest.raises(ValueError):
        svm_engine(sy, t).set_mlp_precision("bf16")
