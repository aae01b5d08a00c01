"""Training the Dense MLP on the device: what the reference's ``create_model`` /
``train_model`` (src/experiments/lcld/model.py:9-42, botnet/model.py:9-47) do with Keras.

``create_model`` draws Keras's Dense defaults (Glorot-uniform kernels, zero biases);
``train_model`` splits off a stratified 10 % validation set, runs Adam on the mean
cross-entropy in batches over one host-drawn permutation per epoch (mv_train_steps) and stops
early on the validation loss (mv_train_eval) like ``EarlyStopping(patience=25)``: no weight
restore, the last epoch's weights are returned.

TensorFlow is absent, so parity with a Keras run is not pinned where it would need Keras's
own random streams or kernels: the shuffle order and the Glorot draws (both come from
``numpy.random.Generator(Philox(seed))`` here), Adam's bias-correction form (Keras's
``lr_t`` form, epsilon outside the square root) and the cross-entropy taken from the logits
(Keras clips the softmax output at 1e-7).  DESIGN.md section 7d.
"""
import numpy as np

from ..attacks.moeva2.classifier import DenseMLPModel
from ..io.tf_bundle import DenseMLP

ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-7)  # Keras's optimizer="adam"


def _generator(seed):
    return np.random.Generator(np.random.Philox(seed))


def glorot_model(dims, seed) -> DenseMLPModel:
    """Dense(relu) ... Dense(softmax) over ``dims`` with Keras's Dense defaults: kernels
    uniform on [-l, l], l = sqrt(6 / (fan_in + fan_out)), biases zero."""
    rng = _generator(seed)
    W, b = [], []
    for k, n in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (k + n))
        W.append(rng.uniform(-lim, lim, (k, n)).astype(np.float32))
        b.append(np.zeros(n, np.float32))
    return DenseMLPModel(DenseMLP(W, b, ["relu"] * (len(dims) - 2) + ["softmax"]))


def class_indices(y) -> np.ndarray:
    """Labels as class indices: (n,) indices or (n, n_classes) one-hot rows."""
    y = np.asarray(y)
    if y.ndim == 2:
        return np.argmax(y, axis=1).astype(np.int32)
    if y.ndim != 1:
        raise ValueError(f"labels of shape {y.shape}: (n,) class indices or (n, classes) one-hot")
    return y.astype(np.int32)


def validation_split(x, y):
    """model.py:24-30: train_test_split(test_size=0.1, random_state=42, stratify=y)."""
    from sklearn.model_selection import train_test_split

    return train_test_split(x, y, test_size=0.1, random_state=42, stratify=y)


class DeviceTrainer:
    """The device side of ``fit``: one epoch of Adam steps and the validation loss."""

    def __init__(self, model, x_train, y_train, x_val, y_val, device=0):
        import torch

        from .._native import Trainer

        mlp = model.dense_weights()
        self.trainer = Trainer(mlp.weights, mlp.biases, device=device, **ADAM)
        dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
        self.x, self.y = up(x_train, np.float32), up(y_train, np.int32)
        self.xv, self.yv = up(x_val, np.float32), up(y_val, np.int32)
        self.out = torch.empty(2, dtype=torch.float32, device=dev)
        self.dev = dev

    def epoch(self, perm, batch_size) -> float:
        """One pass over the training rows in the order ``perm``; the mean of the steps'
        losses (Keras's running training loss weights a short last batch like a full one)."""
        import torch

        n = int(self.x.shape[0])
        n_steps = (n + batch_size - 1) // batch_size
        pd = torch.from_numpy(np.ascontiguousarray(perm, np.int32)).to(self.dev)
        losses = torch.empty(n_steps, dtype=torch.float32, device=self.dev)
        self.trainer.steps(self.x, self.y, batch_size, n_steps, perm=pd, step_losses=losses)
        return float(losses.double().mean().item())

    def validate(self):
        """(validation loss, validation accuracy) of the current weights."""
        self.trainer.eval(self.xv, self.yv, self.out)
        loss, correct = self.out.cpu().numpy().tolist()
        return float(loss), float(correct) / int(self.xv.shape[0])

    def weights(self):
        return self.trainer.get()


def fit(model, x_train_s, y_train, seed=42, epochs=100, batch_size=512, patience=25,
        trainer_factory=DeviceTrainer, return_info=False):
    """``model.fit`` of model.py:31-42 from ``model``'s weights.  ``trainer_factory(model,
    x_train, y_train, x_val, y_val)`` returns an object with ``epoch(perm, batch_size)``,
    ``validate()`` and ``weights()`` (the device trainer; a stub in the CPU tests)."""
    if batch_size < 1 or epochs < 0:
        raise ValueError("batch_size >= 1 and epochs >= 0")
    x = np.asarray(x_train_s, np.float32)
    y = class_indices(y_train)
    if x.ndim != 2 or x.shape[0] != y.shape[0]:
        raise ValueError(f"x {x.shape} and y {y.shape}: one label per row")
    n_out = model.dense_weights().dims[-1]
    if y.min() < 0 or y.max() >= max(n_out, 2):
        raise ValueError(f"labels outside 0..{n_out - 1}")
    x_tr, x_val, y_tr, y_val = validation_split(x, y)
    tr = trainer_factory(model, x_tr, y_tr, x_val, y_val)
    rng = _generator(seed)
    best, wait = np.inf, 0
    info = {"epochs": 0, "train_loss": None, "val_loss": None, "val_accuracy": None,
            "val_losses": [], "stopped_early": False}
    for _ in range(epochs):
        perm = rng.permutation(x_tr.shape[0]).astype(np.int32)
        info["train_loss"] = tr.epoch(perm, batch_size)
        val_loss, val_acc = tr.validate()
        info["epochs"] += 1
        info["val_loss"], info["val_accuracy"] = val_loss, val_acc
        info["val_losses"].append(val_loss)
        # EarlyStopping(monitor="val_loss", mode="min", min_delta=0): np.less(current, best)
        if val_loss < best:
            best, wait = val_loss, 0
        else:
            wait += 1
            if wait >= patience:
                info["stopped_early"] = True
                break
    W, b = tr.weights()
    mlp = model.dense_weights()
    out = DenseMLPModel(DenseMLP([np.asarray(w, np.float32) for w in W],
                                 [np.asarray(v, np.float32) for v in b], list(mlp.activations)))
    return (out, info) if return_info else out
