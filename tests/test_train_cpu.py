"""The host side of training and adversarial retraining (no GPU): initialisation, the
validation split, early stopping on a stub trainer, label forms, save / load, the candidate
filter, and the torch helper against a hand-written backward."""
import numpy as np
import pytest
import torch

import train_torch_ref as tref

from moeva2_amd import defense
from moeva2_amd.attacks.moeva2.classifier import load_model
from moeva2_amd.experiments import training
from moeva2_amd.experiments.botnet import model as botnet_model
from moeva2_amd.experiments.lcld import model as lcld_model


@pytest.mark.parametrize("mod, d, hidden", [(lcld_model, 47, (64, 32, 16, 2)),
                                            (botnet_model, 756, (64, 64, 32, 2))])
def test_create_model_glorot(mod, d, hidden):
    mlp = mod.create_model(d, seed=3).dense_weights()
    assert mlp.dims == [d] + list(hidden)
    assert mlp.activations == ["relu"] * 3 + ["softmax"]
    for w, b in zip(mlp.weights, mlp.biases):
        lim = np.sqrt(6.0 / (w.shape[0] + w.shape[1]))
        assert w.dtype == np.float32 and b.dtype == np.float32
        assert np.abs(w).max() <= lim and np.abs(w).max() > 0.9 * lim  # fills the range
        # uniform on [-lim, lim]: the mean of w.size draws has sigma lim / sqrt(3 size)
        assert abs(float(w.mean())) < 4 * lim / np.sqrt(3 * w.size)
        assert not b.any()
    again = mod.create_model(d, seed=3).dense_weights()
    other = mod.create_model(d, seed=4).dense_weights()
    for w, w2, w3 in zip(mlp.weights, again.weights, other.weights):
        np.testing.assert_array_equal(w, w2)
        assert not np.array_equal(w, w3)


def test_validation_split_is_sklearns():
    from sklearn.model_selection import train_test_split

    x, y = tref.blobs(1000, 5, seed=1)
    y[:700] = 0  # unbalanced: 850 / 150
    x_tr, x_val, y_tr, y_val = training.validation_split(x, y)
    want = train_test_split(x, y, test_size=0.1, random_state=42, stratify=y)
    for got, w in zip((x_tr, x_val, y_tr, y_val), want):
        np.testing.assert_array_equal(got, w)
    assert x_val.shape[0] == 100 and x_tr.shape[0] == 900
    assert int(y_val.sum()) == 15 and int(y_tr.sum()) == 135  # stratified


class StubTrainer:
    """Scripted validation losses; weights() returns the epoch count in every entry."""

    script = []
    made = []

    def __init__(self, model, x_train, y_train, x_val, y_val):
        self.model, self.epochs, self.perms = model, 0, []
        self.shapes = (x_train.shape, y_train.shape, x_val.shape, y_val.shape)
        self.y_train = y_train
        StubTrainer.made.append(self)

    def epoch(self, perm, batch_size):
        assert sorted(perm.tolist()) == list(range(self.shapes[0][0]))
        self.perms.append(perm.copy())
        self.epochs += 1
        return 1.0 / self.epochs

    def validate(self):
        return StubTrainer.script[self.epochs - 1], 0.5

    def weights(self):
        mlp = self.model.dense_weights()
        return ([np.full_like(w, self.epochs) for w in mlp.weights],
                [np.full_like(b, self.epochs) for b in mlp.biases])


def _fit_stub(script, epochs, patience, y=None):
    StubTrainer.script, StubTrainer.made = script, []
    x, y0 = tref.blobs(200, 47, seed=2)
    model, info = lcld_model.train_model(x, y0 if y is None else y, seed=5, epochs=epochs,
                                         batch_size=64, patience=patience, return_info=True,
                                         trainer_factory=StubTrainer)
    return model, info, StubTrainer.made[0]


def test_early_stopping_stops_at_best_plus_patience():
    # best at epoch 3 (index 2), never better again: stops after epoch 3 + 4
    script = [0.9, 0.8, 0.5, 0.6, 0.5, 0.7, 0.55, 0.1, 0.1, 0.1]
    model, info, stub = _fit_stub(script, epochs=10, patience=4)
    assert info["epochs"] == 7 and info["stopped_early"]
    assert info["val_losses"] == script[:7] and info["val_loss"] == script[6]
    # the last epoch's weights, not the best epoch's (no restore)
    assert all((w == 7).all() for w in model.dense_weights().weights)
    assert info["train_loss"] == 1.0 / 7


def test_early_stopping_never_exceeds_epochs():
    model, info, stub = _fit_stub([1.0 / (k + 1) for k in range(50)], epochs=6, patience=2)
    assert info["epochs"] == 6 and not info["stopped_early"] and stub.epochs == 6
    assert all((w == 6).all() for w in model.dense_weights().weights)
    # one permutation per epoch, reproducible per seed, different between epochs
    _, _, again = _fit_stub([1.0 / (k + 1) for k in range(50)], epochs=6, patience=2)
    for p, q in zip(stub.perms, again.perms):
        np.testing.assert_array_equal(p, q)
    assert not np.array_equal(stub.perms[0], stub.perms[1])
    # improving again resets the wait
    _, info, _ = _fit_stub([0.5, 0.6, 0.4, 0.5, 0.3, 0.4, 0.45, 0.2], epochs=8, patience=2)
    assert info["epochs"] == 7


def test_labels_index_and_one_hot():
    x, y = tref.blobs(200, 47, seed=2)
    _, _, a = _fit_stub([0.5], epochs=1, patience=25, y=y)
    _, _, b = _fit_stub([0.5], epochs=1, patience=25, y=np.eye(2)[y])
    assert a.shapes == b.shapes == ((180, 47), (180,), (20, 47), (20,))
    np.testing.assert_array_equal(a.y_train, b.y_train)
    assert a.y_train.dtype == np.int32
    with pytest.raises(ValueError):
        lcld_model.train_model(x, np.full(200, 2), trainer_factory=StubTrainer)
    with pytest.raises(ValueError):
        lcld_model.train_model(x, y[:-1], trainer_factory=StubTrainer)


def test_save_load_round_trip(tmp_path):
    model = botnet_model.create_model(756, seed=9)
    path = model.save(str(tmp_path / "nn"))
    assert path.endswith("nn.npz")
    for p in (path, str(tmp_path / "nn")):
        back = load_model(p).dense_weights()
        assert back.activations == model.dense_weights().activations
        for w, w2 in zip(model.dense_weights().weights, back.weights):
            np.testing.assert_array_equal(w, w2)
            assert w2.dtype == np.float32
        for b, b2 in zip(model.dense_weights().biases, back.biases):
            np.testing.assert_array_equal(b, b2)


def test_candidate_filter():
    """Class 1, predicted 1 at the threshold, every constraint <= 0."""
    class Model:
        def predict_proba(self, xs):
            return np.column_stack([1 - xs[:, 0], xs[:, 0]])

    class Scaler:
        def transform(self, x):
            return x / 10.0

    class Cons:
        def evaluate(self, x):
            return np.column_stack([np.zeros(len(x)), x[:, 1]])

    #              proba*10  cons   label
    x = np.array([[6.0, 0.0],   # 1: kept
                  [6.0, 0.5],   # 1: violates
                  [2.0, 0.0],   # 1: predicted 0 at 0.25? no: 0.2 < 0.25 -> dropped
                  [9.0, 0.0],   # 0: wrong class
                  [2.5, 0.0],   # 1: on the threshold -> kept
                  [7.0, -1.0]])  # one-hot class 1, negative constraint value -> kept
    y = np.array([1, 1, 1, 0, 1, 1])
    rows, idx = defense.select_candidates(Model(), Cons(), Scaler(), x, y, 0.25)
    np.testing.assert_array_equal(idx, [0, 4, 5])
    np.testing.assert_array_equal(rows, x[[0, 4, 5]])
    rows2, idx2 = defense.select_candidates(Model(), Cons(), Scaler(), x, np.eye(2)[y], 0.25)
    np.testing.assert_array_equal(idx2, idx)
    none, idx0 = defense.select_candidates(Model(), Cons(), Scaler(), x, np.zeros(6, int), 0.25)
    assert none.shape == (0, 2) and idx0.size == 0
    with pytest.raises(ValueError):
        defense.adversarial_retrain(Model(), Cons(), Scaler(), x, y, attack="fgsm")


def test_torch_helper_matches_numpy_backward():
    """fp64 autograd equals a hand-written backward to 1e-12 on a 2-layer net, and one Adam
    step of the fp32 helper equals the numpy fp32 statement of the update to 1 ulp."""
    rng = np.random.default_rng(4)
    W = [rng.standard_normal((7, 16)).astype(np.float32), rng.standard_normal((16, 3)).astype(np.float32)]
    b = [rng.standard_normal(16).astype(np.float32), rng.standard_normal(3).astype(np.float32)]
    x = rng.random((29, 7)).astype(np.float32)
    y = rng.integers(0, 3, 29)
    t64 = tref.TrainRef(W, b, torch.float64)
    g, loss = t64.grad(x, y)
    want = tref.numpy_backward(W, b, x, y)
    assert g.shape == want.shape == (7 * 16 + 16 + 16 * 3 + 3,)
    assert np.abs(g - want).max() <= 1e-12
    assert np.abs(want).max() > 1e-3
    # the layout: layer 0's W rows first
    sl = tref.layer_slices([7, 16, 3])
    assert sl[0] == slice(0, 128) and sl[1] == slice(128, 179)
    t32 = tref.TrainRef(W, b, torch.float32)
    g32, _ = t32.grad(x, y)
    w0 = t32.flat()
    t32.step(x, y)
    w1, m1, v1 = tref.adam_numpy_fp32(w0, np.zeros_like(w0), np.zeros_like(w0), g32, 1)
    np.testing.assert_allclose(t32.flat(), w1, rtol=0, atol=float(np.spacing(np.float32(4.0))))
    np.testing.assert_array_equal(t32.flat_state()[0], m1)
    assert np.abs(w1 - w0).max() > 5e-4  # the first Adam step moves by about lr


def test_exported_symbols_include_training():
    from moeva2_amd import _native

    for s in ("mv_train_create", "mv_train_steps", "mv_train_eval", "mv_train_grad",
              "mv_train_get", "mv_train_get_state", "mv_train_set_state", "mv_train_destroy"):
        assert s in _native.EXPORTED
