"""Training on the device (mv_train_*) against the torch CPU restatement
(tests/train_torch_ref.py), and adversarial retraining end to end.

Tolerances follow DESIGN.md section 7a: the floor of a comparison is the fp32 helper's own
error against the fp64 helper on the test's inputs (bounded below by 2^-23 relative), the
engine is allowed 4x that floor, and no row or parameter is left out.  Gradient and parameter
errors are relative to the layer's (W and b together) inf-norm in the fp64 helper, losses to
1 + |loss|.  DESIGN.md section 7d lists the measured floors and engine errors.

Inputs are the C-PGD tests' ``perturbed_typed`` rows (33 LCLD, 17 botnet), tiled to the batch
size, with labels drawn over the classes so that softmax - onehot takes both signs.  Batch
sizes are the tile and workgroup edges: 1, 15, 16, 17; 64 and 65 (the LCLD plan's four tiles
per workgroup, then a second workgroup with one live row); 512 and 513; and 16400, where 1025
tiles exceed 256 workgroups of four waves and every plan takes two tiles per wave.
"""
import os

import numpy as np
import pytest
import torch

import pgd_torch_ref as ref
import test_gpu_pgd as tp
import train_torch_ref as tref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EPS23 = 2.0 ** -23
BATCHES = [1, 15, 16, 17, 64, 65, 512, 513, 16400]
NETS = ["lcld", "botnet"] + [n for n in tp.NETS]
REFUSED = [(47, 24, 2), (47, 528, 2), (47, 16, 9), (47, 16, 16, 16, 16, 16, 16, 2)]

_CASES, _MODELS = {}, {}


def _case(project):
    if project not in _CASES:
        _CASES[project] = tp.Case(project, engine=False)
    return _CASES[project]


def _net_id(p):
    return p if isinstance(p, str) else "x".join(map(str, p[0]))


class Model:
    """One net: weights, its input rows, the helpers' factories."""

    def __init__(self, param):
        if isinstance(param, str):
            s = ref.Spec(param, F32)
            self.W, self.b = [w.numpy() for w in s.W], [v.numpy() for v in s.b]
            self.rows = _case(param).inputs["perturbed_typed"]
            seed = 100
        else:
            dims, seed = param
            self.W, self.b = tp.synthetic_net(dims, seed)
            self.rows = _case("lcld").inputs["perturbed_typed"]
        self.dims = [self.W[0].shape[0]] + [w.shape[1] for w in self.W]
        self.seed = seed
        self.slices = tref.layer_slices(self.dims)
        self._trainer = None

    def data(self, n, seed=0):
        x = tp._tiled(self.rows, n)
        y = np.random.default_rng(self.seed + seed).integers(0, self.dims[-1], n).astype(np.int32)
        return x, y

    def helper(self, dtype):
        return tref.TrainRef(self.W, self.b, dtype)

    def trainer(self, fresh=False):
        from moeva2_amd._native import Trainer

        if fresh:
            return Trainer(self.W, self.b)
        if self._trainer is None:
            self._trainer = Trainer(self.W, self.b)
        return self._trainer

    def layer_err(self, got, want64):
        """max over layers of |got - want| / the layer's inf-norm in want."""
        got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
        return max(float(np.abs(got[s] - want64[s]).max() / max(np.abs(want64[s]).max(), 1e-30))
                   for s in self.slices)


def _model(param):
    key = _net_id(param)
    if key not in _MODELS:
        _MODELS[key] = Model(param)
    return _MODELS[key]


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _dev_grad(tr, xd, yd, perm=None):
    g = torch.empty(tr.n_params, dtype=torch.float32, device="cuda")
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    tr.grad(xd, yd, g, loss, perm=perm)
    torch.cuda.synchronize()
    return g.cpu().numpy(), float(loss.cpu().numpy()[0])


def _state(tr):
    W, b = tr.get()
    m, v, t = tr.get_state()
    return tref.flatten(W, b), m, v, t


def _loss_err(got, want):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    return float(np.max(np.abs(got - want) / (1 + np.abs(want))))


# ---- 1. weight gradient ----------------------------------------------------------------------

@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("net", NETS, ids=_net_id)
def test_weight_gradient_matches_fp64_autograd(net, n):
    mdl = _model(net)
    x, y = mdl.data(n)
    g64, l64 = mdl.helper(F64).grad(x, y)
    g32, l32 = mdl.helper(F32).grad(x, y)
    g, loss = _dev_grad(mdl.trainer(), _dev(x, np.float32), _dev(y, np.int32))
    assert np.isfinite(g).all() and np.isfinite(loss)
    floor_g = max(mdl.layer_err(g32, g64), EPS23)
    floor_l = max(_loss_err(l32, l64), EPS23)
    err_g, err_l = mdl.layer_err(g, g64), _loss_err(loss, l64)
    print(f"train grad {_net_id(net)} n {n}: gradient err {err_g:.3e} (floor {floor_g:.3e}), "
          f"loss err {err_l:.3e} (floor {floor_l:.3e})")
    assert err_g <= 4 * floor_g
    assert err_l <= 4 * floor_l
    if mdl.dims[-1] == 1:
        assert not g.any() and loss == 0
    else:  # both signs of softmax - onehot reach the last bias, and every layer has gradient
        assert all(np.abs(g64[s]).max() > 0 for s in mdl.slices)


# ---- 2. padding ------------------------------------------------------------------------------

@pytest.mark.parametrize("net", ["lcld", "botnet"])
def test_padding_contributes_nothing(net):
    mdl = _model(net)
    tr = mdl.trainer()
    x, y = mdl.data(32)
    xd, yd = _dev(x, np.float32), _dev(y, np.int32)
    g17, l17 = _dev_grad(tr, _dev(x[:17], np.float32), _dev(y[:17], np.int32))
    g17b, l17b = _dev_grad(tr, xd[:17], yd[:17])  # the same rows inside the 32-row buffer
    np.testing.assert_array_equal(g17, g17b)
    assert l17 == l17b
    g32, _ = _dev_grad(tr, xd, yd)
    assert not np.array_equal(g32, g17)
    xn = x.copy()
    xn[16:] = np.nan
    g16, l16 = _dev_grad(tr, _dev(x[:16], np.float32), _dev(y[:16], np.int32))
    g16n, l16n = _dev_grad(tr, _dev(xn, np.float32)[:16], yd[:16])
    assert np.isfinite(g16n).all() and np.isfinite(l16n)
    np.testing.assert_array_equal(g16, g16n)
    assert l16 == l16n


# ---- 3. Adam ---------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("net", ["lcld", "botnet"])
def test_adam_update_bit_identical(net, t):
    """One step from known (w, m, v, t) equals the numpy fp32 statement of the update fed with
    the device's own mv_train_grad output."""
    mdl = _model(net)
    tr = mdl.trainer(fresh=True)
    x, y = mdl.data(64, seed=3)
    xd, yd = _dev(x, np.float32), _dev(y, np.int32)
    rng = np.random.default_rng(t)
    if t > 1:
        m0 = (1e-3 * rng.standard_normal(tr.n_params)).astype(np.float32)
        v0 = (1e-6 * rng.random(tr.n_params)).astype(np.float32)
        tr.set_state(m0, v0, t - 1)
    w0, m0, v0, t0 = _state(tr)
    assert t0 == t - 1
    g, _ = _dev_grad(tr, xd, yd)
    tr.steps(xd, yd, 64, 1)
    w1, m1, v1, t1 = _state(tr)
    ww, wm, wv = tref.adam_numpy_fp32(w0, m0, v0, g, t)
    assert t1 == t
    np.testing.assert_array_equal(m1, wm)
    np.testing.assert_array_equal(v1, wv)
    np.testing.assert_array_equal(w1, ww)
    assert np.abs(w1 - w0).max() > 1e-4


# ---- 4. and 6. trajectory, reproducibility -----------------------------------------------------

def _perms(n, epochs, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.permutation(n).astype(np.int32) for _ in range(epochs)]


def _device_trajectory(mdl, x, y, batch, perms):
    tr = mdl.trainer(fresh=True)
    xd, yd = _dev(x, np.float32), _dev(y, np.int32)
    per = (x.shape[0] + batch - 1) // batch
    losses = torch.empty(per * len(perms), dtype=torch.float32, device="cuda")
    for e, p in enumerate(perms):
        tr.steps(xd, yd, batch, per, perm=None if p is None else _dev(p, np.int32),
                 step_losses=losses[e * per:(e + 1) * per])
    torch.cuda.synchronize()
    return _state(tr), losses.cpu().numpy()


def _helper_trajectory(mdl, dtype, x, y, batch, perms):
    h = mdl.helper(dtype)
    per = (x.shape[0] + batch - 1) // batch
    losses = np.concatenate([h.steps(x, y, batch, per, perm=p) for p in perms])
    return h, losses


@pytest.mark.parametrize("net", ["lcld", "botnet"])
def test_trajectory_and_reproducibility(net):
    """20 steps (5 epochs of 4: 64, 64, 64 and 8 rows of 200) from the shipped weights;
    parameters and step losses by the floor rule; a second run is bit-identical."""
    mdl = _model(net)
    x, y = mdl.data(200, seed=5)
    perms = _perms(200, 5)
    h32, l32 = _helper_trajectory(mdl, F32, x, y, 64, perms)
    h64, l64 = _helper_trajectory(mdl, F64, x, y, 64, perms)
    w64 = h64.flat()
    floor_w = max(mdl.layer_err(h32.flat(), w64), EPS23)
    floor_l = max(_loss_err(l32, l64), EPS23)
    # the test tells something: every layer moved by far more than the tolerance
    w_init = tref.flatten(mdl.W, mdl.b)
    moved = min(float(np.abs(w64[s] - w_init[s]).max() / np.abs(w64[s]).max()) for s in mdl.slices)
    print(f"train trajectory {net}: helper floor params {floor_w:.3e} losses {floor_l:.3e}, "
          f"least-moved layer {moved:.3e}")
    assert moved > 1000 * 4 * floor_w
    (w, m, v, t), losses = _device_trajectory(mdl, x, y, 64, perms)
    assert t == 20 and losses.shape == (20,)
    err_w, err_l = mdl.layer_err(w, w64), _loss_err(losses, l64)
    print(f"train trajectory {net}: engine err params {err_w:.3e} losses {err_l:.3e}")
    assert err_w <= 4 * floor_w
    assert err_l <= 4 * floor_l
    (w2, m2, v2, t2), losses2 = _device_trajectory(mdl, x, y, 64, perms)
    for a, b in ((w, w2), (m, m2), (v, v2), (losses, losses2)):
        np.testing.assert_array_equal(a, b)


# ---- 5. batching and permutation -------------------------------------------------------------

def test_short_last_batch_divides_by_its_size():
    mdl = _model("lcld")
    x, y = mdl.data(1000, seed=7)
    h32, l32 = _helper_trajectory(mdl, F32, x, y, 512, [None])
    h64, l64 = _helper_trajectory(mdl, F64, x, y, 512, [None])
    floor_w = max(mdl.layer_err(h32.flat(), h64.flat()), EPS23)
    floor_l = max(_loss_err(l32, l64), EPS23)
    tr = mdl.trainer(fresh=True)
    xd, yd = _dev(x, np.float32), _dev(y, np.int32)
    losses = torch.empty(2, dtype=torch.float32, device="cuda")
    tr.steps(xd, yd, 512, 2, step_losses=losses)
    w = _state(tr)[0]
    err_w, err_l = mdl.layer_err(w, h64.flat()), _loss_err(losses.cpu().numpy(), l64)
    print(f"train short batch: params err {err_w:.3e} (floor {floor_w:.3e}), losses err "
          f"{err_l:.3e} (floor {floor_l:.3e})")
    assert err_w <= 4 * floor_w and err_l <= 4 * floor_l
    # dividing the 488-row step by 512 instead would scale its loss by 488 / 512
    assert abs(l64[1]) * (1 - 488 / 512) / (1 + abs(l64[1])) > 1000 * 4 * floor_l


@pytest.mark.parametrize("net", ["lcld", "botnet"])
def test_perm_and_step_grouping_bit_identical(net):
    mdl = _model(net)
    x, y = mdl.data(200, seed=9)
    perm = _perms(200, 1, seed=11)[0]
    base, lb = _device_trajectory(mdl, x, y, 64, [perm])
    host, lh = _device_trajectory(mdl, x[perm], y[perm], 64, [None])
    tr = mdl.trainer(fresh=True)  # perm = NULL on the host-permuted rows, one step per call
    xd, yd = _dev(x[perm], np.float32), _dev(y[perm], np.int32)
    losses = torch.empty(4, dtype=torch.float32, device="cuda")
    for s in range(4):
        tr.steps(xd, yd, 64, 1, first_row=64 * s, step_losses=losses[s:s + 1])
    single = _state(tr)
    for got in (host, single):
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(lb, lh)
    np.testing.assert_array_equal(lb, losses.cpu().numpy())
    unpermuted, _ = _device_trajectory(mdl, x, y, 64, [np.arange(200, dtype=np.int32)])
    assert not np.array_equal(unpermuted[0], base[0])  # the order matters


# ---- 7. evaluation ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [33, 1000, 16400])
@pytest.mark.parametrize("net", ["lcld", "botnet"])
def test_eval_loss_and_count(net, n):
    mdl = _model(net)
    x, y = mdl.data(n, seed=13)
    l64, c64, margin = mdl.helper(F64).eval(x, y)
    l32, _, _ = mdl.helper(F32).eval(x, y)
    assert margin.min() > 1e-4  # no row's label hangs on fp32 rounding: none is left out
    out = torch.empty(2, dtype=torch.float32, device="cuda")
    mdl.trainer().eval(_dev(x, np.float32), _dev(y, np.int32), out)
    loss, correct = out.cpu().numpy().tolist()
    floor = max(_loss_err(l32, l64), EPS23)
    err = _loss_err(loss, l64)
    print(f"train eval {net} n {n}: loss err {err:.3e} (floor {floor:.3e}), correct {correct:.0f} "
          f"of {n}, least margin {margin.min():.3e}")
    assert err <= 4 * floor
    assert correct == c64 and 0 < c64 < n


# ---- 8. it learns ----------------------------------------------------------------------------

def test_learns_blobs():
    from moeva2_amd.experiments import training
    from moeva2_amd.experiments.lcld.model import create_model

    x, y = tref.blobs(2048, 47, seed=0)
    model = create_model(47, seed=0)
    mlp = model.dense_weights()
    x_tr, x_val, y_tr, y_val = training.validation_split(x, y)
    rng = np.random.Generator(np.random.Philox(0))
    perms = [rng.permutation(x_tr.shape[0]).astype(np.int32) for _ in range(5)]
    vals = {}
    for dt in (F32, F64):
        h = tref.TrainRef(mlp.weights, mlp.biases, dt)
        vals[dt] = []
        for p in perms:
            h.steps(x_tr, y_tr, 512, 4, perm=p)
            vals[dt].append(h.eval(x_val, y_val))
    v32, v64 = (np.array([v[0] for v in vals[dt]]) for dt in (F32, F64))
    margin = vals[F64][-1][2]
    close = int((margin <= 1e-4).sum())
    print(f"train blobs: rows with fp64 margin <= 1e-4: {close}")
    assert close == 0
    new, info = training.fit(model, x, y, seed=0, epochs=5, batch_size=512, return_info=True)
    got = np.array(info["val_losses"])
    floor = max(_loss_err(v32, v64), EPS23)
    err = _loss_err(got, v64)
    print(f"train blobs: val loss per epoch {got}, err {err:.3e} (floor {floor:.3e}), accuracy "
          f"{info['val_accuracy']:.4f} (helper {vals[F64][-1][1] / len(y_val):.4f})")
    assert info["epochs"] == 5 and err <= 4 * floor
    assert round(info["val_accuracy"] * len(y_val)) == vals[F64][-1][1]
    assert got[-1] < got[0] and v64[-1] < v64[0]  # it learns


# ---- 9. train_model / adversarial_retrain end to end --------------------------------------------

def test_adversarial_retrain_end_to_end(tmp_path):
    from moeva2_amd import defense
    from moeva2_amd.attacks.moeva2.classifier import Classifier, load_model
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.attacks.moeva2.objective_calculator import ObjectiveCalculator
    from moeva2_amd.experiments.united.moeva_run import NpzScaler
    from moeva2_amd.experiments.united.utils import get_constraints_from_str

    res = ref.RES
    feat = os.path.join(res, "data", "lcld", "features.csv")
    c = get_constraints_from_str("lcld")(feat, feat.replace("features", "constraints"))
    scaler = NpzScaler(os.path.join(res, "models", "lcld", "scaler.npz"))
    model = load_model(os.path.join(res, "models", "lcld", "nn.npz"))
    x1 = np.load(os.path.join(res, "data", "lcld", "x_candidates_synthetic.npy"))[:8]
    xb, yb = tref.blobs(128, 47, seed=0)
    x0 = (xb[yb == 0].astype(np.float64) - scaler.min_) / scaler.scale_
    x = np.concatenate([x1, x0])
    y = np.concatenate([np.ones(8, np.int32), np.zeros(64, np.int32)])
    kw = dict(attack="moeva", threshold=0.25, eps=0.2, norm=2, budget=20, seed=42, epochs=3)
    new, info = defense.adversarial_retrain(model, c, scaler, x, y, **kw)
    print(f"adversarial_retrain: {info}")
    pop = info["generated_per_candidate"]
    assert 0 < info["candidates"] <= 8
    assert 0 <= info["successes"] <= info["candidates"] * pop
    assert info["retrain_rows"] == 72 + info["successes"] and info["base_rows"] == 72
    assert info["epochs"] == 3 and np.isfinite(info["train_loss"]) and np.isfinite(info["val_loss"])
    assert new.dense_weights().dims == model.dense_weights().dims
    back = load_model(new.save(str(tmp_path / "robust"))).dense_weights()
    for a, b in zip(new.dense_weights().weights + new.dense_weights().biases,
                    back.weights + back.biases):
        np.testing.assert_array_equal(a, b)
    again, info2 = defense.adversarial_retrain(model, c, scaler, x, y, **kw)
    for a, b in zip(new.dense_weights().weights + new.dense_weights().biases,
                    again.dense_weights().weights + again.dense_weights().biases):
        np.testing.assert_array_equal(a, b)
    assert info2 == info
    # both attacks accept the new model; the same seeded attack before and after (printed, not
    # asserted: three epochs on 72 rows harden nothing)
    cand, _ = defense.select_candidates(model, c, scaler, x, y, 0.25)
    rates = {}
    for name, mdl in (("before", model), ("after", new)):
        gen = defense.attack_moeva(mdl, c, scaler, cand, 2, 20, 42)
        assert gen.shape == (len(cand), pop, 47) and np.isfinite(gen).all()
        calc = ObjectiveCalculator(Classifier(mdl), c, minimize_class=1,
                                   thresholds={"f1": 0.25, "f2": 0.2}, min_max_scaler=scaler,
                                   ml_scaler=scaler, norm=2)
        ok = calc.get_successful_attacks(cand, gen, preferred_metrics="misclassification",
                                         order="asc", max_inputs=1)
        rates[name] = len(ok) / len(cand)
    print(f"adversarial_retrain: MoEvA2 success rate before {rates['before']:.3f}, after "
          f"{rates['after']:.3f}")
    assert rates["before"] * len(cand) == info["successes"]
    adv = defense.attack_pgd(new, c, scaler, cand, 2, 7, 0.2)
    assert adv.shape == (len(cand), 1, 47) and np.isfinite(adv).all()
    assert isinstance(Moeva2(new, c, ml_scaler=scaler)._get_classifier(), Classifier)


# ---- 10. refusals ----------------------------------------------------------------------------

@pytest.mark.parametrize("dims", REFUSED, ids=["width24", "width528", "outputs9", "layers7"])
def test_create_refusals(dims):
    from moeva2_amd._native import NativeError, Trainer

    W, b = tp.synthetic_net(dims, 1)
    with pytest.raises(NativeError, match="error 1: mv_train_create"):
        Trainer(W, b)


def test_step_refusals():
    from moeva2_amd._native import NativeError

    mdl = _model("lcld")
    tr = mdl.trainer(fresh=True)
    x, y = mdl.data(33)
    xd, yd = _dev(x, np.float32), _dev(y, np.int32)
    w0 = _state(tr)
    for kw in (dict(batch=0, n_steps=1), dict(batch=-4, n_steps=1),
               dict(batch=16, n_steps=1, first_row=33), dict(batch=16, n_steps=1, first_row=-1),
               dict(batch=16, n_steps=4)):  # the fourth step would start at row 48
        with pytest.raises(NativeError, match="error 1: mv_train_steps"):
            tr.steps(xd, yd, **kw)
    for a, b in zip(w0, _state(tr)):
        np.testing.assert_array_equal(a, b)
    tr.steps(xd, yd, 16, 3)  # 16, 16 and 1 rows
    assert _state(tr)[3] == 3
