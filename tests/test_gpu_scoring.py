"""The scoring kernels (csrc/objectives.hip: k_objectives, k_obj_mlscale) at their shape
edges.  The shipped problems give them two feature counts, at most a handful of one-hot groups
and row counts far below the grid cap, so no lane loop took a second trip in the suite.

1. ``ObjCalc.score`` on synthetic arrays (no problem, no model) against a plain fp64 statement
   of objective_calculator.py:44-84 whose sums are exactly rounded (``math.fsum``): CV and the
   L2 f2 at 1e-12 relative (a wave reduction of at most a few hundred
   non-negative terms is far inside it), the Linf f2 and f1 bit for bit (a maximum and a copy
   round nothing).  Cases move one parameter at a time: D, C (0 with a null G), the number of
   one-hot groups (sizes 1..4, the last group owning the last feature, groups whose sum is
   not 1), the batch shape (B * n mod 4, one row, workgroups that straddle two states), the
   classifier outputs, both norms; then the CV sign rule, a NaN column and the range flag at
   its inclusive bounds.
2. the whole ``mv_objcalc_run`` chain on two problems of tests/synth_problem.py: ``run`` equals
   ``score`` fed by the same constraint engine and ``Mlp.predict`` on a host-scaled ML row, bit
   for bit, with and without an ML scaler, once with B * n * D above k_obj_mlscale's grid
   (8192 x 256 threads); the success rates of a short attack against the oracle.
"""
import math

import numpy as np
import pytest

import synth_problem as sp
from oracle import moeva_oracle as mo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LO, HI = 0.0 - 1e-4, 1.0 + 1e-4  # objective_calculator.py:72-76, inclusive
# report only: the worst relative error against the exact sums seen so far in this process,
# printed by check(); the 1e-12 assertions are what pins the values
WORST = {"cv": 0.0, "f2": 0.0}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ 1. synthetic arrays
def make_groups(D, n_ohe, rng):
    """n_ohe disjoint one-hot groups of 1..4 features over the last features of the row, in
    shuffled order; the last group holds feature D - 1."""
    sizes = [1 + g % 4 for g in range(n_ohe)]
    tot = sum(sizes)
    assert tot <= D
    ids = D - tot + rng.permutation(tot)
    if n_ohe:
        k = int(np.where(ids == D - 1)[0][0])
        ids[k], ids[-1] = ids[-1], ids[k]
    cuts = np.cumsum([0] + sizes)
    return [ids[cuts[g]:cuts[g + 1]].astype(np.int32) for g in range(n_ohe)]


class Arrays:
    """Seeded inputs of one score call.  The one-hot features keep mm_scale 1 / mm_min 0 and
    hold multiples of 1/8 in [0, 1], so a group's sum and |1 - sum| are exact in any order;
    about a third of the groups do not sum to 1.  Every other feature scales into
    [mm_min, mm_min + 0.8] inside [0, 1].  G mixes positive values over twelve decades,
    negative ones, 0.0 and -0.0."""

    def __init__(self, D, C, n_ohe, B, n, n_out, seed):
        rng = np.random.default_rng(seed)
        self.D, self.C, self.B, self.n, self.n_out = D, C, B, n, n_out
        self.groups = make_groups(D, n_ohe, rng)
        ohe = (np.concatenate(self.groups) if n_ohe else np.zeros(0, np.int32)).astype(int)
        self.mm_scale = rng.uniform(0.05, 0.5, D)
        self.mm_min = rng.uniform(0.0, 0.2, D)
        self.mm_scale[ohe], self.mm_min[ohe] = 1.0, 0.0
        span = 0.8 / self.mm_scale
        self.x_init = rng.uniform(0.0, 1.0, (B, D)) * span
        x = self.x_init[:, None, :] + rng.normal(0.0, 0.1, (B, n, D)) * span
        x = np.clip(x, 0.0, span)
        for q, g in enumerate(self.groups):
            hot = g[rng.integers(0, len(g), (B, n))]
            x[..., g] = 0.0
            np.put_along_axis(x, hot[..., None], 1.0, axis=2)
            if q % 3 == 1:  # a sum below 1: 0 .. 0.75
                x[..., g[0]] = rng.integers(0, 4, (B, n)) / 8.0
                x[..., g[1:]] = rng.integers(0, 2, (B, n, len(g) - 1)) / 8.0
            elif q % 6 == 2:  # every member hot: the sum is the group's size
                x[..., g] = 1.0
        self.x_init[:, ohe] = x[:, 0][:, ohe]
        if n > 1:
            x[:, 0] = self.x_init  # one exact origin per state: f2 == 0
        self.x = x
        G = rng.standard_normal((B * n, C)) * 10.0 ** rng.integers(-9, 4, (B * n, C))
        kind = rng.integers(0, 6, (B * n, C))
        G[kind == 0] = 0.0
        G[kind == 1] = -0.0
        self.G = G if C else None
        p = rng.uniform(0.0, 1.0, (B * n, n_out))
        self.proba = p if n_out == 1 else p / p.sum(axis=1, keepdims=True)


def reference(a, cls, norm):
    """objective_calculator.py:44-84 in fp64, the sums exactly rounded."""
    rows = a.x.reshape(a.B * a.n, a.D)
    xs = rows * a.mm_scale
    xs = xs + a.mm_min  # MinMaxScaler.transform: two roundings
    xi = a.x_init * a.mm_scale
    xi = xi + a.mm_min
    d = np.repeat(xi, a.n, axis=0) - xs
    obj = np.empty((a.B * a.n, 3))
    for r in range(rows.shape[0]):
        cols = [] if a.G is None else list(a.G[r])
        cols.append(math.fsum(abs(1.0 - math.fsum(rows[r, g])) for g in a.groups))
        cols = np.array(cols)
        # Problem.calc_constraint_violation: sum(G * (G > 0)); NaN * False is NaN
        obj[r, 0] = np.nan if np.isnan(cols).any() else math.fsum(cols[cols > 0])
        if norm == 2:
            obj[r, 2] = math.sqrt(math.fsum(d[r] * d[r]))
        else:
            obj[r, 2] = np.abs(d[r]).max()
    p = a.proba
    # Classifier.predict_proba: a one-column model means [1 - p, p]
    obj[:, 1] = (1.0 - p[:, 0] if cls == 0 else p[:, 0]) if a.n_out == 1 else p[:, cls]
    bad = ~((xs >= LO) & (xs <= HI)).all(axis=1)
    bad |= np.repeat(~((xi >= LO) & (xi <= HI)).all(axis=1), a.n)
    return obj, bad.astype(np.int32)


def score(a, cls, norm):
    """ObjCalc.score on the arrays; obj and the flags start as NaN / -1, so a row the
    kernel does not write cannot pass."""
    from moeva2_amd._native import ObjCalc

    oc = ObjCalc(a.D, a.groups, a.mm_scale, a.mm_min, norm=norm)
    dev = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v), device="cuda")  # noqa: E731
    obj = torch.full((a.B, a.n, 3), float("nan"), dtype=torch.float64, device="cuda")
    bad = torch.full((a.B, a.n), -1, dtype=torch.int32, device="cuda")
    oc.score(dev(a.x_init), dev(a.x), dev(a.G), dev(a.proba), cls, obj, bad)
    torch.cuda.synchronize()
    return obj.cpu().numpy().reshape(-1, 3), bad.cpu().numpy().reshape(-1)


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.int64)


def check(a, cls, norm, what, f2_rows=None):
    obj, bad = score(a, cls, norm)
    ref, ref_bad = reference(a, cls, norm)
    rows = np.arange(obj.shape[0]) if f2_rows is None else f2_rows
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, col in (("cv", 0), ("f2", 2)):
            r = rows if col == 2 else np.arange(obj.shape[0])
            err = np.abs(obj[r, col] - ref[r, col]) / np.abs(ref[r, col])
            err = err[np.isfinite(err)]
            if err.size:
                WORST[k] = max(WORST[k], float(err.max()))
    print(f"{what}: worst relative error so far CV {WORST['cv']:.3e}, f2 {WORST['f2']:.3e}")
    np.testing.assert_array_equal(bad, ref_bad, err_msg=f"{what}: range_bad")
    np.testing.assert_allclose(obj[:, 0], ref[:, 0], rtol=1e-12, atol=0, err_msg=f"{what}: CV")
    np.testing.assert_array_equal(_bits(obj[:, 1]), _bits(ref[:, 1]), err_msg=f"{what}: f1")
    if norm == 2:
        np.testing.assert_allclose(obj[rows, 2], ref[rows, 2], rtol=1e-12, atol=0,
                                   err_msg=f"{what}: f2")
    else:
        np.testing.assert_array_equal(obj[rows, 2], ref[rows, 2], err_msg=f"{what}: f2")
    return obj, bad, ref


def _d_for(n_ohe):
    return sum(1 + g % 4 for g in range(n_ohe)) + 3


# (id, D, C, n_ohe, B, n, n_out, cls): one parameter moves, the others stay small
SHAPES = (
    [(f"D{D}", D, 3, 1 if D == 1 else 3, 3, 3, 2, 1) for D in (1, 63, 64, 65, 129)]
    + [(f"C{C}", 9, C, 2, 3, 3, 2, 1) for C in (0, 1, 64, 65, 130)]
    + [(f"ohe{g}", _d_for(g), 3, g, 3, 3, 2, 1) for g in (0, 1, 64, 65, 130)]
    # B * n mod 4 = 1, 2, 1, 3, 3, 0, 1: one row; workgroups of four rows over two states
    + [(f"B{B}n{n}", 9, 3, 2, B, n, 2, 1)
       for B, n in ((1, 1), (3, 2), (3, 3), (5, 3), (3, 5), (4, 6), (3, 7))]
    + [(f"out{o}c{c}", 9, 3, 2, 3, 3, o, c)
       for o, c in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 2), (8, 7))]
    # every lane loop on its second or third trip at once
    + [("all", _d_for(130) + 2, 130, 130, 5, 7, 3, 2)]
)


@pytest.mark.parametrize("norm", [2, np.inf], ids=["l2", "linf"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_score_shapes(shape, norm):
    name, D, C, n_ohe, B, n, n_out, cls = shape
    a = Arrays(D, C, n_ohe, B, n, n_out, seed=100 + [s[0] for s in SHAPES].index(name))
    obj, bad, ref = check(a, cls, norm, f"{name} norm {norm}")
    assert not bad.any()
    if n > 1:
        assert (obj.reshape(B, n, 3)[:, 0, 2] == 0.0).all()  # the exact origins (row / n)
    if n_ohe > 1:
        assert (ref[:, 0] > 0).all()  # a group off 1 in every row


@pytest.mark.parametrize("n_ohe", [0, 3, 65])
def test_cv_sign_rule(n_ohe):
    """Success is CV <= 0: a row whose columns are all <= 0 (-0.0 included) has CV exactly 0.0,
    one column of 1e-300 (in the second 64-lane trip) makes it positive, and so does one
    one-hot group an ulp off 1."""
    C = 65
    a = Arrays(_d_for(n_ohe), C, n_ohe, 2, 5, 2, seed=7)
    for g in a.groups:  # every group sums to exactly 1
        a.x[..., g] = 0.0
        a.x[..., g[-1]] = 1.0
    a.G = -np.abs(a.G)
    a.G[:, ::3] = -0.0
    a.G[:, 1::3] = 0.0
    tiny_rows, ohe_rows = [1, 6, 9], [2, 7] if n_ohe else []
    for r in tiny_rows:
        a.G[r, 64] = 1e-300
    rows = a.x.reshape(-1, a.D)
    for q, r in enumerate(ohe_rows):  # the last group (feature D - 1 among its members)
        g = a.groups[-1]
        rows[r, g[-1]] = np.nextafter(1.0, 0.0) if q == 0 else 0.5
    obj, _, ref = check(a, 1, 2, f"sign rule n_ohe {n_ohe}")
    zero = np.setdiff1d(np.arange(10), tiny_rows + ohe_rows)
    assert (_bits(obj[zero, 0]) == 0).all(), obj[:, 0]  # +0.0, bit for bit
    assert (obj[tiny_rows, 0] == 1e-300).all(), obj[:, 0]
    if n_ohe:
        assert obj[2, 0] == 1.0 - np.nextafter(1.0, 0.0) and obj[7, 0] == 0.5, obj[:, 0]


@pytest.mark.parametrize("col", [0, 64, 129])
def test_cv_nan_column_stays_in_its_row(col):
    a = Arrays(9, 130, 2, 3, 3, 2, seed=11)
    a.G[4, col] = np.nan
    obj, _, ref = check(a, 1, 2, f"NaN in G column {col}")
    assert np.isnan(obj[4, 0]) and np.isfinite(np.delete(obj[:, 0], 4)).all()


_OUT = {"lo": (LO, 0), "hi": (HI, 0), "below": (np.nextafter(LO, -np.inf), 1),
        "above": (np.nextafter(HI, np.inf), 1), "nan": (np.nan, 1)}


@pytest.mark.parametrize("where", ["x", "x_init"])
@pytest.mark.parametrize("kind", list(_OUT))
def test_range_flag_bounds(where, kind):
    """The scaling asserts are inclusive at 0 - 1e-4 and 1 + 1e-4: a scaled value exactly there
    is not flagged, one ulp outside (or a NaN) is.  D 65 puts feature D - 1 alone in the second
    lane trip; 3 x 3 rows leave the last row alone in the last workgroup.  mm_scale 1 and
    mm_min 0 on the features used make the stored value the scaled value.  A flag is its row's
    own (a state's rows for x_init)."""
    value, flag = _OUT[kind]
    D, B, n = 65, 3, 3
    for feat, row in ((D - 1, B * n - 1), (0, 4), (D - 1, 0), (63, B * n - 1)):
        a = Arrays(D, 3, 0, B, n, 2, seed=13)
        a.mm_scale[[0, 63, D - 1]], a.mm_min[[0, 63, D - 1]] = 1.0, 0.0
        a.x_init[:, [0, 63, D - 1]] = 0.5
        a.x[..., [0, 63, D - 1]] = 0.25
        want = np.zeros(B * n, np.int32)
        if where == "x":
            a.x.reshape(-1, D)[row, feat] = value
            want[row] = flag
        else:
            a.x_init[row // n, feat] = value
            want[row // n * n:(row // n + 1) * n] = flag
        ok = np.where(want == 0)[0]
        _, bad, _ = check(a, 1, 2, f"range {where} {kind} feature {feat} row {row}", f2_rows=ok)
        np.testing.assert_array_equal(bad, want)


# ------------------------------------------------------------------ 2. the run chain
NARROW, WIDE = "n8f", "o40f"  # D 23 with one-hot groups of 2 and 5; D 77 (a partial second trip)
BIG_ROWS = 11000              # x 3 states x D 77 = 2,541,000 elements > 8192 x 256


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth_scoring")
    cache = {}

    def get(name):
        if name not in cache:
            sy = sp.build(name, d)
            xl, xu = sy.bounds()
            lo, hi = xl.min(axis=0), xu.max(axis=0)
            scale = np.where(hi > lo, 1.0 / np.where(hi > lo, hi - lo, 1.0), 1.0)
            sy.mm = sp.Scaler(scale, -lo * scale)  # min-max over the states' bounds
            sy.xl, sy.xu = xl, xu
            cache[name] = sy
        return cache[name]

    return get


def calculator(sy, ml, norm=2, thr=(0.5, 0.6)):
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator
    from moeva2_amd.io.tf_bundle import DenseMLP

    if not hasattr(sy, "clf"):
        sy.clf = Classifier(DenseMLPModel(DenseMLP(sy.W, sy.bs, ["relu", "relu", "softmax"])))
    return ObjectiveCalculator(sy.clf, sy.constraints, 1, {"f1": thr[0], "f2": thr[1]},
                               min_max_scaler=sy.mm, norm=norm, ml_scaler=sy.scaler if ml else None)


def candidates(sy, n, seed):
    """(B, n, D) rows inside each state's bounds, one member hot per one-hot group."""
    from moeva2_amd.attacks.moeva2.utils import get_ohe_masks

    rng = np.random.default_rng(seed)
    x = rng.uniform(sy.xl[:, None, :], sy.xu[:, None, :], (sp.B, n, sy.D))
    for m in get_ohe_masks(sy.types):
        g = np.asarray(m)
        hot = g[rng.integers(0, len(g), (sp.B, n))]
        x[..., g] = 0.0
        np.put_along_axis(x, hot[..., None], 1.0, axis=2)
    x[:, 0] = sy.X
    return x


def run_and_score(sy, x, ml):
    """(obj, flags) of ObjCalc.run and of ObjCalc.score on the same rows."""
    calc = calculator(sy, ml)
    oc, ceng, mlp = calc._device()
    assert ceng is not None and mlp is not None
    B, n, D = x.shape
    xi, xd = torch.as_tensor(sy.X, device="cuda"), torch.as_tensor(x, device="cuda")
    out = []
    for _ in range(2):
        out.append((torch.full((B, n, 3), float("nan"), dtype=torch.float64, device="cuda"),
                    torch.full((B, n), -1, dtype=torch.int32, device="cuda")))
    oc.run(ceng, mlp, xi, xd, 1, *out[0])
    G = torch.empty((B * n, ceng.prog.C), dtype=torch.float64, device="cuda")
    ceng.constraints(xd.view(B * n, D), G)
    x_ml = x.reshape(B * n, D)
    if ml:
        x_ml = x_ml * sy.ml[0]
        x_ml = x_ml + sy.ml[1]
    proba = torch.empty((B * n, 2), dtype=torch.float64, device="cuda")
    mlp.predict(torch.as_tensor(np.ascontiguousarray(x_ml), device="cuda"), proba)
    oc.score(xi, xd, G, proba, 1, *out[1])
    torch.cuda.synchronize()
    return [(o.cpu().numpy().reshape(-1, 3), b.cpu().numpy().reshape(-1)) for o, b in out]


def assert_rows_equal(run, sc, what):
    (ro, rb), (so, sb) = run, sc
    last = ro.shape[0] - 1
    assert not np.isnan(so[:, 1:]).any() and (sb >= 0).all()
    diff = np.where((_bits(ro) != _bits(so)).any(axis=1) | (rb != sb))[0]
    assert diff.size == 0, (
        f"{what}: run != score on {diff.size} of {last + 1} rows, first {diff[0]}, last "
        f"{diff[-1]}; row 0 run {ro[0]} score {so[0]}; row {last} run {ro[last]} score {so[last]}")


@pytest.mark.parametrize("ml", [True, False], ids=["ml_scaler", "no_ml_scaler"])
@pytest.mark.parametrize("name", [NARROW, WIDE])
def test_run_equals_score(built, name, ml):
    sy = built(name)
    run, sc = run_and_score(sy, candidates(sy, 7, 21), ml)  # 21 rows: B * n mod 4 = 1
    assert_rows_equal(run, sc, f"{name} ml {ml}")
    # the classifier saw another row with the scaler than without
    assert np.unique(run[0][:, 1]).size > 3


def test_run_equals_score_above_the_mlscale_grid(built):
    """B * n * D = 2,541,000 > 8192 x 256: the elements past 2,097,152 are scaled by the second
    trip of k_obj_mlscale's grid-stride loop and reach f1 only."""
    sy = built(WIDE)
    assert sp.B * BIG_ROWS * sy.D > 8192 * 256 and (sp.B * BIG_ROWS) % 4 == 0
    x = candidates(sy, BIG_ROWS, 22)
    run, sc = run_and_score(sy, x, True)
    assert_rows_equal(run, sc, f"{WIDE} at {sp.B * BIG_ROWS} rows (first 0, last {sp.B * BIG_ROWS - 1})")
    first_tail = 8192 * 256 // sy.D  # the first row with an element of the second trip
    assert np.unique(run[0][first_tail:, 1]).size > 1000


@pytest.mark.parametrize("norm", [2, np.inf], ids=["l2", "linf"])
def test_success_rates_against_oracle(built, norm):
    """A short attack's final populations (decoded to ML rows) through
    ObjectiveCalculator.success_rate_3d and through the oracle's restatement."""
    from test_gpu_row_routes import run_attack

    sy = built(NARROW)
    _, g, _, _ = run_attack(sy, "two_point", hist=0)
    xs = np.stack([mo.genetic_to_ml(sy.lay, g[b], sy.X[b]) for b in range(sp.B)])
    xs[:, 0] = sy.X
    thr = (0.5, 0.6)
    calc = calculator(sy, True, norm, thr)
    obj = calc.calculate_objectives_3d(sy.X, xs)

    def fn(xi, x):
        return mo.objectives_calc(xi, x, sy.constraints_fn, sy.types, sy.ml[0], sy.ml[1], sy.W,
                                  sy.bs, 1, sy.mm.scale_, sy.mm.min_,
                                  "inf" if norm == np.inf else 2)

    for b in range(sp.B):
        ref = fn(sy.X[b], xs[b])
        np.testing.assert_allclose(obj[b][:, 0], ref[:, 0], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(obj[b][:, 1], ref[:, 1], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(obj[b][:, 2], ref[:, 2], rtol=1e-12, atol=1e-15)
        # no candidate sits on a threshold, so the two sides cannot disagree by rounding
        assert (np.abs(ref[:, 1] - thr[0]) > 1e-4).all()
        assert (np.abs(ref[:, 2] - thr[1]) > 1e-9).all()
    got, want = calc.success_rate_3d(sy.X, xs), mo.success_rate_3d(sy.X, xs, fn, *thr)
    np.testing.assert_array_equal(got, want)
    print(f"success rates o1..o7 (norm {norm}): {got}")
