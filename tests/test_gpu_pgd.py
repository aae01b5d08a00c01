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

The second half of the module covers what the invariants cannot: every loop mode against the
helper over 14 (and 9) iterations, so that the adaptive step table, the repair inside the loop,
norm inf, the constraints-only loss and caller-supplied labels are arithmetic that is compared
(floors 2^-23 .. 4.0e-7 without repair, 1.4e-6 .. 1.5e-5 with it; engine at most 2.4e-7); rows
independent of batch size, tile position and tiles per workgroup (bit-exact, n up to 16384);
and five synthetic classifier shapes that take the column-tile guards, the second column pass,
the streamed first layer and 1, 3 and 8 classes.
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

    def __init__(self, project, engine=True):
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
        # engine=False: the inputs and torch references alone (no device object)
        self.est = TF2Classifier(self.model, self.c, self.scaler,
                                 parameters={"constraints_optim": "sum"}) if engine else None
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

    def run(self, x, mode, norm, max_iter, y=None, batch_size=1 << 20, est=None):
        from moeva2_amd.attacks.pgd.atk import PGDTF2

        return PGDTF2(est or self.est, norm=norm, eps=EPS, eps_step=0.1, max_iter=max_iter,
                      batch_size=batch_size, loss_evaluation=mode).generate(x, y=y, mask=self.mask)

    def traj(self, which, mode, norm, max_iter, y=None, spec=None, tag=None):
        """The helper's (fp32, fp64) results of one attack, computed once.  spec: a
        (fp32, fp64) pair of Specs in place of the shipped net's; tag names it and y."""
        key = ("traj", which, mode, norm, max_iter, tag)
        if key not in self.refs:
            self.refs[key] = tuple(
                s.attack(self.inputs[which], self.mask, mode, norm, EPS, max_iter,
                         ohe_groups=self.groups, y=y).numpy()
                for s in (spec or (self.s32, self.s64)))
        return self.refs[key]


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


# ---- loop modes, multi-tile workgroups and classifier shapes --------------------------------
#
# A trajectory is compared with the helper in fp32 under the rule of test_trajectory_norm2:
# inf-norm error <= 4 x max(the helper's own fp32-vs-fp64 divergence on the same inputs,
# 2^-23).  A row the two helpers themselves disagree on by more than 1e-4 (a label or a
# gradient sign decided by fp32 rounding) is left out; the helpers alone define that set, and
# its size is bounded per test.

ROW_DIVERGED = 1e-4
HEADLINE = "constraints+flip+adaptive_eps_step+repair"
_L = "lcld"
_B = "botnet"
# (project, inputs, mode, norm, max_iter): max_iter 14 -> iter_per_step 2, step table entries
# 0..6; max_iter 9 -> iter_per_step 1, entries 0..8
LOOP = (
    [(_L, "perturbed_typed", "constraints", norm, 14) for norm in (np.inf, 2)]
    + [(_L, which, mode, norm, 14)
       for which in ("candidates", "perturbed_typed")
       for mode in ("constraints+flip", "constraints+flip+adaptive_eps_step", HEADLINE,
                    "flip+repair")
       for norm in (np.inf, 2)]
    + [(_L, "perturbed_typed", HEADLINE, np.inf, 9)]
    + [(_B, "candidates", mode, np.inf, 14)
       for mode in ("constraints", "constraints+adaptive_eps_step",
                    "constraints+adaptive_eps_step+repair")]
    + [(_B, "perturbed_typed", "constraints", norm, 14) for norm in (np.inf, 2)]
    + [(_B, "perturbed_typed", mode, 2, 14)
       for mode in ("constraints+flip", "constraints+flip+adaptive_eps_step", HEADLINE)]
)
MAX_EXCLUDED = {_L: 0, _B: 2}


def _get(project):
    if project not in _CASES:
        _CASES[project] = Case(project)
    return _CASES[project]


def _loop_id(p):
    return f"{p[0]}-{p[1]}-{p[2]}-norm{p[3]}-it{p[4]}"


def _row_div(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(1)


def _kept_rows(name, t32, t64, max_excluded):
    """(rows the two helpers agree on, tolerance); asserts the bound on the excluded share."""
    div = _row_div(t32, t64)
    keep = div <= ROW_DIVERGED
    excluded = int((~keep).sum())
    floor = max(float(div[keep].max()) if keep.any() else 0.0, 2.0 ** -23)
    print(f"{name}: helper fp32-vs-fp64 floor {floor:.3e}, excluded rows {excluded} of "
          f"{len(keep)}")
    assert excluded <= max_excluded
    return keep, 4 * floor


def _assert_matches(name, got, t32, keep, tol):
    assert np.isfinite(got).all()
    err = float(_row_div(got[keep], t32[keep]).max())
    print(f"{name}: engine err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


def strip_mode(mode, word):
    return "+".join(w for w in mode.split("+") if w != word)


@pytest.mark.parametrize("p", LOOP, ids=_loop_id)
def test_loop_modes(p):
    """Every loop mode against the torch restatement: adaptive step table (with iter_per_step
    2 and 1), repair inside the loop, norm inf over many iterations, the constraints-only
    loss.  The helper-only checks come first: the adaptive result is far from the
    constant-step one on every row, and on the LCLD candidates repair moves >= 30 of 33
    rows; so a kernel that ignored either would leave the tolerance."""
    project, which, mode, norm, max_iter = p
    case = _get(project)
    name = _loop_id(p)
    t32, t64 = case.traj(which, mode, norm, max_iter)
    keep, tol = _kept_rows(name, t32, t64, MAX_EXCLUDED[project])
    if "adaptive_eps_step" in mode:
        const = case.traj(which, strip_mode(mode, "adaptive_eps_step"), norm, max_iter)[0]
        gap = _row_div(t32, const)
        print(f"{name}: adaptive vs constant step, per-row gap {gap.min():.3e} .. {gap.max():.3e}")
        assert gap.min() > 1000 * tol
    if "repair" in mode and project == _L and which == "candidates" and "adaptive" in mode:
        plain = case.traj(which, strip_mode(mode, "repair"), norm, max_iter)[0]
        moved = int((_row_div(t32, plain) > tol).sum())
        print(f"{name}: repair changes {moved} of {len(plain)} rows")
        assert moved >= 30
    got = case.run(case.inputs[which], mode, norm, max_iter)
    _assert_matches(name, got, t32, keep, tol)


def test_explicit_labels():
    """Caller-supplied y (the complement of the fp64 prediction): neither side predicts, the
    result matches the helper and differs from the y = None result."""
    case = _get(_L)
    # the shipped candidates: on the perturbed rows one row's sign pattern is decided by fp32
    # rounding under these labels (the helpers alone diverge there by 7.5e-2)
    which, mode = "candidates", "constraints+flip"
    y = (1 - case.y[which]).astype(np.int32)
    t32, t64 = case.traj(which, mode, 2, 14, y=y, tag="complement")
    keep, tol = _kept_rows("explicit labels", t32, t64, 0)
    own = case.traj(which, mode, 2, 14)[0]
    assert _row_div(t32, own).min() > 1000 * tol
    got = case.run(case.inputs[which], mode, 2, 14, y=y)
    _assert_matches("explicit labels", got, t32, keep, tol)
    assert _row_div(got, case.run(case.inputs[which], mode, 2, 14)).min() > 1000 * tol


@pytest.mark.parametrize("norm", [np.inf, 2])
def test_small_batches(case, norm):
    """max_iter 0 returns the input; n = 1 (partial tile), 15 (one short) and 16 (exact tile)
    give the rows of the full run bit for bit."""
    x = case.inputs["perturbed_typed"]
    # (the adaptive step needs max_iter >= 7)
    np.testing.assert_array_equal(case.run(x, "constraints+flip+repair", norm, 0), x)
    full = case.run(x, HEADLINE, norm, 7)
    assert not np.array_equal(full, x)
    for n in (1, 15, 16):
        np.testing.assert_array_equal(case.run(x[:n], HEADLINE, norm, 7), full[:n])
        # and from the middle of the batch: another position in the tile
        np.testing.assert_array_equal(case.run(x[16 - n:16], HEADLINE, norm, 7), full[16 - n:16])


def _tiled(x, n):
    return np.ascontiguousarray(x[np.arange(n) % x.shape[0]])


@pytest.mark.parametrize("norm", [np.inf, 2])
@pytest.mark.parametrize("n", [8193, 12293, 16384])
def test_tiles_per_workgroup_lcld(n, norm):
    """2, 3 (dead waves in the last workgroup) and 4 tiles per workgroup: a row's result does
    not depend on its wave's LDS slice, the block that staged the weights or its position."""
    case = _get(_L)
    x = case.inputs["perturbed_typed"]
    base = case.run(x, HEADLINE, norm, 7)
    assert not np.array_equal(base, x)
    got = case.run(_tiled(x, n), HEADLINE, norm, 7)
    np.testing.assert_array_equal(got, _tiled(base, n))


def test_tiles_per_workgroup_grad():
    """k_pgd_grad with 2 tiles per workgroup: gradient and all 2 + C loss columns."""
    case = _get(_L)
    x, y = case.inputs["perturbed_typed"], case.y["perturbed_typed"]
    g0, l0 = case.est.losses_and_gradient(x, y, "constraints+flip")
    g, losses = case.est.losses_and_gradient(_tiled(x, 8193), _tiled(y, 8193), "constraints+flip")
    assert losses.shape == (8193, 2 + case.c.get_nb_constraints())
    np.testing.assert_array_equal(g, _tiled(g0, 8193))
    np.testing.assert_array_equal(losses, _tiled(l0, 8193))
    assert np.abs(g0).max() > 0


def test_tiles_per_workgroup_botnet():
    """n = 8193 plans 2 tiles per workgroup and falls back to 1 on the LDS limit (one botnet
    wave tile is ~116 KB)."""
    case = _get(_B)
    x = case.inputs["perturbed_typed"]
    base = case.run(x, "constraints+flip", 2, 3)
    assert not np.array_equal(base, x)
    np.testing.assert_array_equal(case.run(_tiled(x, 8193), "constraints+flip", 2, 3),
                                  _tiled(base, 8193))


@pytest.mark.parametrize("norm", [np.inf, 2])
def test_batch_size(norm):
    """Three launches of 16, 16 and 1 rows equal one launch of 33."""
    case = _get(_L)
    x = case.inputs["perturbed_typed"]
    np.testing.assert_array_equal(case.run(x, HEADLINE, norm, 7, batch_size=16),
                                  case.run(x, HEADLINE, norm, 7))


def test_repair_three_blocks():
    """fix_features_types on 300 rows (k_pgd_repair: two full 128-thread blocks and one of
    44) equals the 33-row result, which test_repair compares with the helper."""
    case = _get(_L)
    xf = case.s32.unscale(torch.tensor(case.inputs["perturbed"])).numpy().astype(np.float32)
    base = case.c.fix_features_types(xf)
    assert not np.array_equal(base, xf)
    np.testing.assert_array_equal(case.c.fix_features_types(_tiled(xf, 300)), _tiled(base, 300))


# (shape, seed): the LCLD constraints and scaler around synthetic classifiers
NETS = [
    ((47, 16, 2), 11),                     # one hidden layer, one column tile
    ((47, 48, 112, 16, 32, 16, 3), 12),    # 6 layers, widest in the middle, 3 and 7 tiles
    ((47, 512, 8), 13),                    # first layer streamed (too large for LDS), 8 classes
    ((47, 128, 80, 2), 14),                # two column passes: 8 - 4, then 5 - 4 tiles
    ((47, 32, 1), 15),                     # one output: loss 0, gradient exactly 0
]
MAX_EXCLUDED_NET = 3


def synthetic_net(dims, seed):
    """He-normal weights N(0, 2 / fan_in), biases 0.1 N(0, 1), fp32."""
    rng = np.random.default_rng(seed)
    W = [(rng.standard_normal((k, n)) * np.sqrt(2.0 / k)).astype(np.float32)
         for k, n in zip(dims[:-1], dims[1:])]
    b = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in dims[1:]]
    return W, b


class Net:
    """One synthetic classifier on the LCLD case: torch Specs, labels, the device estimator."""

    def __init__(self, dims, seed, engine=True):
        self.dims, self.case = dims, _get(_L) if engine else Case(_L, engine=False)
        self.W, self.b = synthetic_net(dims, seed)
        self.spec = tuple(ref.Spec(_L, dt, self.W, self.b) for dt in (torch.float32, torch.float64))
        self.y_rand = np.random.default_rng(seed + 1000).integers(
            0, dims[-1], self.case.inputs["perturbed"].shape[0]).astype(np.int32)
        self.y_pred = self.spec[1].predict(
            self.case.inputs["perturbed_typed"]).numpy().astype(np.int32)
        self.est = None
        if engine:
            from moeva2_amd.attacks.moeva2.classifier import DenseMLPModel
            from moeva2_amd.attacks.pgd.classifier import TF2Classifier
            from moeva2_amd.io.tf_bundle import DenseMLP

            acts = ["relu"] * (len(dims) - 2) + ["softmax"]
            model = DenseMLPModel(DenseMLP(self.W, self.b, acts))
            self.est = TF2Classifier(model, self.case.c, self.case.scaler,
                                     parameters={"constraints_optim": "sum"})


_NETS = {}


@pytest.fixture(params=NETS, ids=lambda p: "x".join(map(str, p[0])))
def net(request):
    if request.param not in _NETS:
        _NETS[request.param] = Net(*request.param)
    return _NETS[request.param]


def test_net_gradient(net):
    """Mode flip (a constraint term would set the row's gradient scale and hide an MLP
    error), labels drawn over the classes: gradient relative to the row's inf-norm and
    loss_class relative to 1 + |loss|, each within 4x the helper's fp32-vs-fp64 floor."""
    x, y = net.case.inputs["perturbed"], net.y_rand
    g32, lc32 = (v.numpy() for v in net.spec[0].grad(x, y, "flip")[:2])
    g64, lc64 = (v.numpy() for v in net.spec[1].grad(x, y, "flip")[:2])
    g, losses = net.est.losses_and_gradient(x, y, "flip")
    assert np.isfinite(g).all() and np.isfinite(losses).all()
    gs = np.maximum(np.abs(g64).max(1, keepdims=True), 1e-30)
    ls = 1 + np.abs(lc64)
    floor_g = max(_rel(g32, g64, gs), 2.0 ** -23)
    floor_l = max(_rel(lc32, lc64, ls), 2.0 ** -23)
    err_g, err_l = _rel(g, g64, gs), _rel(losses[:, 0], lc64, ls)
    print(f"net {net.dims}: gradient err {err_g:.3e} (floor {floor_g:.3e}), loss_class err "
          f"{err_l:.3e} (floor {floor_l:.3e})")
    assert err_g <= 4 * floor_g
    assert err_l <= 4 * floor_l
    if net.dims[-1] == 1:
        assert not g.any() and not losses[:, 0].any()
    else:
        assert np.abs(g).max(1).min() > 0


@pytest.mark.parametrize("norm", [np.inf, 2])
def test_net_trajectory(net, norm):
    """10 iterations of mode flip from the type-valid rows, labels given (the fp64
    prediction), under the rule of test_loop_modes; at most 3 of 33 rows excluded."""
    case = net.case
    name = f"net {net.dims} norm {norm}"
    t32, t64 = case.traj("perturbed_typed", "flip", norm, 10, y=net.y_pred, spec=net.spec,
                         tag=net.dims)
    keep, tol = _kept_rows(name, t32, t64, MAX_EXCLUDED_NET)
    got = case.run(case.inputs["perturbed_typed"], "flip", norm, 10, y=net.y_pred, est=net.est)
    _assert_matches(name, got, t32, keep, tol)
    if net.dims[-1] == 1:
        np.testing.assert_array_equal(got, case.inputs["perturbed_typed"])
    else:
        assert _row_div(t32, case.inputs["perturbed_typed"]).min() > 1000 * tol  # every row moves


@pytest.mark.parametrize("dims", [(47, 24, 2), (47, 528, 2), (47, 16, 9),
                                  (47, 16, 16, 16, 16, 16, 16, 2), (46, 16, 2)],
                         ids=["width24", "width528", "outputs9", "layers7", "input46"])
def test_create_refusals(dims):
    from moeva2_amd._native import NativeError, Pgd

    case = _get(_L)
    W, b = synthetic_net(dims, 1)
    with pytest.raises(NativeError, match="mv_pgd_create"):
        Pgd(case.c.tensor_program(), W, b, case.scaler.scale_, case.scaler.min_, case.mask,
            *case.c.tensor_repair())
