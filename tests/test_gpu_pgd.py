"""C-PGD on the device against the torch CPU restatement (tests/pgd_torch_ref.py).

Shapes: LCLD n = 33 (two full 16-row tiles and a 1-row tail), botnet n = 17; the shipped
candidates and a fixed-seed perturbation of them inside the feature bounds (active constraint
columns, no row on a tie of ``minimum``).

Tolerances are 4x the helper's own fp32-vs-fp64 error on the same inputs (the engine's MFMA
summation order differs from torch's), measured when the module's references are built.
Measured floors (max over rows, gradient error relative to the row's gradient inf-norm;
losses / columns relative to 1 + the row's largest value): gradient 4.9e-7 .. 2.8e-6 on LCLD
(2.0 on the shipped LCLD candidates with a constraint term, where a column within fp32
rounding of tol flips its sign), 8.4e-8 .. 1.2e-2 on botnet; losses 6.9e-3 / 6.7e-4 (LCLD),
1.2e-7 / 7.4e-7 (botnet); 10-iteration trajectory 1.6e-7 / 1.2e-7; repair installment 3.6e-6
relative.  DESIGN.md section 7a lists them with the engine's measured errors.

The invariants are checked from initial states the attack is given in use: rows whose typed
features are valid (the shipped candidates, and the perturbed rows passed once through the
torch restatement of fix_features_types).  The eps bound is a bound on the distance to
x_init, and the specified repair runs after the projection: from a row with a fractional term
or a one-hot group that is not one-hot, the repair alone moves the row by its own distance to
validity (0.315 in scaled L2 on the raw perturbed LCLD rows, eps 0.2, engine and torch
restatement alike), which says nothing about the attack.
"""
import json
import os

import numpy as np
import pytest
import torch

import pgd_torch_ref as ref

pytestmark = pytest.mark.gpu

RES = ref.RES
N = {"lcld": 33, "botnet": 17}
MODES = ["flip", "constraints", "constraints+flip"]
SWEEP = ["flip", "constraints+flip", "constraints+flip+adaptive_eps_step",
         "constraints+flip+adaptive_eps_step+repair"]
EPS = 0.2 - 1e-6


class Case:
    """One project's inputs, engine objects and torch references, built once."""

    def __init__(self, project):
        from moeva2_amd.attacks.moeva2.classifier import load_model
        from moeva2_amd.attacks.pgd.classifier import TF2Classifier
        from moeva2_amd.experiments.united.moeva_run import NpzScaler
        from moeva2_amd.experiments.united.utils import get_constraints_from_str

        self.project = project
        feat = os.path.join(RES, "data", project, "features.csv")
        self.c = get_constraints_from_str(project)(feat, feat.replace("features", "constraints"))
        name = {"lcld": "x_candidates_synthetic.npy", "botnet": "x_candidates_common.npy"}[project]
        x = np.load(os.path.join(RES, "data", project, name), allow_pickle=False)[:N[project]]
        rng = np.random.default_rng(7)
        lo, hi = self.c.feature_min_max_batch(x)
        xp = x + 0.1 * (lo + rng.random(x.shape) * (hi - lo) - x)
        self.scaler = NpzScaler(os.path.join(RES, "models", project, "scaler.npz"))
        self.model = load_model(os.path.join(RES, "models", project, "nn.npz"))
        self.est = TF2Classifier(self.model, self.c, self.scaler,
                                 parameters={"constraints_optim": "sum"})
        self.mask = np.asarray(self.c.get_mutable_mask()).astype(bool)
        self.groups = self.c.tensor_repair()[0]
        self.s32, self.s64 = ref.Spec(project, torch.float32), ref.Spec(project, torch.float64)
        # scaled fp32 rows, inside the clip range
        self.inputs = {k: np.clip(self.scaler.transform(v), 0, 1).astype(np.float32)
                       for k, v in (("candidates", x), ("perturbed", xp))}
        # the perturbed rows with valid typed features (a fixed point of the repair): term on
        # {36, 60}, installment recomputed, one-hot groups one-hot; botnet: unchanged
        typed = self.s32.rescale(self.s32.repair(
            self.s32.unscale(torch.tensor(self.inputs["perturbed"])), self.groups)).numpy()
        self.inputs["perturbed_typed"] = np.clip(typed, 0, 1).astype(np.float32)
        self.y = {k: self.s64.predict(v).numpy().astype(np.int32) for k, v in self.inputs.items()}
        self.refs = {}

    def grad_refs(self, which, mode):
        key = (which, mode)
        if key not in self.refs:
            x, y = self.inputs[which], self.y[which]
            self.refs[key] = (self.s64.grad(x, y, mode), self.s32.grad(x, y, mode))
        return self.refs[key]

    def run(self, x, mode, norm, max_iter, y=None):
        from moeva2_amd.attacks.pgd.atk import PGDTF2

        return PGDTF2(self.est, norm=norm, eps=EPS, eps_step=0.1, max_iter=max_iter,
                      batch_size=1 << 20, loss_evaluation=mode).generate(x, y=y, mask=self.mask)


_CASES = {}


@pytest.fixture(params=["lcld", "botnet"])
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param)
    return _CASES[request.param]


def _rel(got, want, scale):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    err = np.where(both_nan, 0.0, np.abs(got - want))
    return float(np.max(err / scale))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["candidates", "perturbed"])
def test_gradient_matches_fp64_autograd(case, which, mode):
    """mv_pgd_grad vs fp64 autograd: gradient (relative to the row's gradient inf-norm), both
    losses and all C columns (relative to 1 + the row's largest |value|), each within 4x the
    helper's own fp32-vs-fp64 error on these rows."""
    (g64, lc64, cs64, col64), (g32, lc32, cs32, col32) = case.grad_refs(which, mode)
    g, losses = case.est.losses_and_gradient(case.inputs[which], case.y[which], mode)
    assert np.isfinite(g).all()
    gs = np.maximum(np.abs(g64.numpy()).max(1, keepdims=True), 1e-30)
    cs = 1 + np.maximum(np.abs(col64.numpy()).max(1, keepdims=True), np.abs(lc64.numpy())[:, None])
    ref_l = np.column_stack([lc64.numpy(), cs64.numpy(), col64.numpy()])
    f32_l = np.column_stack([lc32.numpy(), cs32.numpy(), col32.numpy()])
    floor_g = max(_rel(g32.numpy(), g64.numpy(), gs), 2.0 ** -23)
    floor_l = max(_rel(f32_l, ref_l, cs), 2.0 ** -23)
    err_g, err_l = _rel(g, g64.numpy(), gs), _rel(losses, ref_l, cs)
    print(f"{case.project} {which} {mode}: gradient err {err_g:.3e} (floor {floor_g:.3e}), "
          f"losses err {err_l:.3e} (floor {floor_l:.3e})")
    assert losses.shape == (N[case.project], 2 + case.c.get_nb_constraints())
    assert err_g <= 4 * floor_g
    assert err_l <= 4 * floor_l


@pytest.mark.parametrize("norm", [np.inf, 2])
def test_update_rule_one_iteration(case, norm):
    """max_iter 1: x_adv equals the specified step, clip and projection applied on the host in
    fp32 to the engine's own gradient: exactly for norm inf, within 2 ulp for norm 2."""
    x, y = case.inputs["perturbed"], case.y["perturbed"]
    g, _ = case.est.losses_and_gradient(x, y, "constraints+flip")
    # the host statement sums a row in the kernel's order (pgd_torch_ref.step_device_order)
    want = ref.step_device_order(x, x, g, case.mask, norm, EPS, 0.1)
    got = case.run(x, "constraints+flip", norm, 1, y=y)
    if norm == np.inf:
        np.testing.assert_array_equal(got, want)
    else:
        # x_adv = x_init + d is rounded at the magnitude of its larger operand, so the ulp is
        # taken there (an entry clipped to ~0 from x_init = 0.05 carries ulp(0.05) of error)
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(x)).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want) / np.maximum(ulp, 2.0 ** -149)
        print(f"{case.project} update rule norm 2: max error {err.max():.2f} ulp")
        assert err.max() <= 2
    assert not np.array_equal(got, x)


def test_trajectory_norm2(case):
    """10 iterations, norm 2, against the helper in fp32; tolerance 4x the helper's own
    fp32-vs-fp64 divergence after the same 10 iterations (inf-norm over all entries)."""
    x = case.inputs["perturbed"]
    mode = "constraints+flip"
    t32 = case.s32.attack(x, case.mask, mode, 2, EPS, 10).numpy()
    t64 = case.s64.attack(x, case.mask, mode, 2, EPS, 10).numpy()
    floor = max(float(np.abs(t32 - t64).max()), 2.0 ** -23)
    got = case.run(x, mode, 2, 10)
    err = float(np.abs(got - t32).max())
    print(f"{case.project} trajectory: err {err:.3e} (fp32-vs-fp64 floor {floor:.3e})")
    assert err <= 4 * floor


@pytest.mark.parametrize("norm", [np.inf, 2])
@pytest.mark.parametrize("mode", SWEEP)
@pytest.mark.parametrize("which", ["candidates", "perturbed_typed"])
def test_invariants(case, which, mode, norm):
    """All four sweep modes, both norms, from type-valid initial states (module docstring):
    0 <= x_adv <= 1, ||x_adv - x_init|| <= eps (1 + 1e-6), immutable features bit-identical
    when repair is off, a zero mask returns the input."""
    x = case.inputs[which]
    got = case.run(x, mode, norm, 7)
    assert np.isfinite(got).all()
    assert got.min() >= 0 and got.max() <= 1
    d = got.astype(np.float64) - x
    dist = np.abs(d).max(1) if norm == np.inf else np.sqrt((d * d).sum(1))
    print(f"{case.project} {which} {mode} norm {norm}: min {got.min():.9g} max {got.max():.9g} "
          f"dist {dist.max():.9g} (eps {EPS:.9g})")
    assert dist.max() <= EPS * (1 + 1e-6)
    if "repair" not in mode:
        np.testing.assert_array_equal(got[:, ~case.mask], x[:, ~case.mask])
    assert not np.array_equal(got, x)
    from moeva2_amd.attacks.pgd.atk import PGDTF2

    zero = PGDTF2(case.est, norm=norm, eps=EPS, max_iter=7, loss_evaluation=mode).generate(
        x, mask=np.zeros_like(case.mask))
    np.testing.assert_array_equal(zero, x)


def test_repair(case):
    """fix_features_types on perturbed feature-space rows equals the helper: term and one-hot
    groups exactly, the installment within 4x the fp32 pow floor (helper fp32 vs fp64)."""
    xf = case.s32.unscale(torch.tensor(case.inputs["perturbed"])).numpy().astype(np.float32)
    got = case.c.fix_features_types(xf)
    if case.project == "botnet":
        np.testing.assert_array_equal(got, xf)
        return
    w32 = case.s32.repair(torch.tensor(xf), case.groups).numpy()
    w64 = case.s64.repair(torch.tensor(xf, dtype=torch.float64), case.groups).numpy()
    keep = np.ones(xf.shape[1], bool)
    keep[3] = False
    np.testing.assert_array_equal(got[:, keep], w32[:, keep])
    assert set(np.unique(got[:, 1])) <= {36.0, 60.0}
    for m in case.groups:
        assert (got[:, m].sum(1) == 1).all()
    floor = max(float(np.max(np.abs(w32[:, 3] - w64[:, 3]) / np.abs(w64[:, 3]))), 2.0 ** -23)
    err = float(np.max(np.abs(got[:, 3] - w64[:, 3]) / np.abs(w64[:, 3])))
    print(f"repair installment: err {err:.3e} (floor {floor:.3e})")
    assert err <= 4 * floor


def test_surface(case):
    """evaluate(use_tensors=True) returns the losses columns; PGDTF2.generate is mv_pgd_run."""
    from moeva2_amd._native import PGD_LOSS_CONSTRAINTS, PGD_LOSS_FLIP

    x = case.inputs["perturbed"]
    xf = case.s32.unscale(torch.tensor(x)).numpy().astype(np.float32)
    cols = case.c.evaluate(xf, use_tensors=True)
    assert cols.dtype == np.float32 and cols.shape == (x.shape[0], case.c.get_nb_constraints())
    want = ref.Spec(case.project, torch.float64).constraints(
        torch.tensor(xf, dtype=torch.float64)).numpy()
    f32 = case.s32.constraints(torch.tensor(xf)).numpy()
    scale = 1 + np.abs(want).max(1, keepdims=True)
    floor = max(_rel(f32, want, scale), 2.0 ** -23)
    assert _rel(cols, want, scale) <= 4 * floor
    assert (cols > 0).any()
    xd = torch.from_numpy(x).cuda()
    xa = torch.empty_like(xd)
    case.est.pgd.run(xd, xa, 7, 2, EPS, 0.1, PGD_LOSS_FLIP | PGD_LOSS_CONSTRAINTS)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(case.run(x, "constraints+flip", 2, 7), xa.cpu().numpy())


def test_driver_lcld(tmp_path):
    from moeva2_amd.attacks.moeva2.classifier import Classifier, load_model
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator
    from moeva2_amd.experiments.united import pgd_run
    from moeva2_amd.experiments.united.moeva_run import load_scaler, resolve_path

    cfg = {"attack_name": "pgd", "comet": False, "constraints_optim": "sum",
           "project_name": "lcld", "loss_evaluation": "constraints+flip+adaptive_eps_step+repair",
           "budget": 7, "eps": 0.2, "norm": 2, "seed": 42, "misclassification_threshold": 0.25,
           "n_initial_state": 33, "initial_state_offset": 0, "reconstruction": False,
           "save_history": "none", "system": {"n_jobs": 1, "verbose": 0},
           "dirs": {"results": str(tmp_path)},
           "paths": {"model": "./models/lcld/nn.model", "features": "./data/lcld/features.csv",
                     "constraints": "./data/lcld/constraints.csv",
                     "x_candidates": "./data/lcld/x_candidates_synthetic.npy",
                     "ml_scaler": "./models/lcld/scaler.joblib"}}
    metrics = pgd_run.run(cfg, verbose=False)
    paths = pgd_run.output_paths(cfg)
    for p in paths.values():
        assert os.path.exists(p), p
    xa = np.load(paths["x_attacks"])
    assert xa.shape == (33, 1, 47)
    c = _CASES["lcld"].c if "lcld" in _CASES else Case("lcld").c
    x0 = np.load(resolve_path(cfg["paths"]["x_candidates"]))[:33]
    scaler = load_scaler(cfg["paths"]["ml_scaler"])
    calc = ObjectiveCalculator(Classifier(load_model(resolve_path(cfg["paths"]["model"]))), c,
                               minimize_class=1, thresholds={"f1": 0.25, "f2": 0.2},
                               min_max_scaler=scaler, ml_scaler=scaler, norm=2)
    df = calc.success_rate_3d_df(x0, xa)
    import pandas as pd

    saved = pd.read_csv(paths["success_rate"])
    np.testing.assert_allclose(saved.values, df.values, rtol=0, atol=1e-12)
    with open(paths["metrics"]) as f:
        m = json.load(f)
    assert m["objectives"] == metrics["objectives"] == df.to_dict(orient="records")[0]
    assert pgd_run.run(cfg, verbose=False) is None  # idempotent skip
