"""C-PGD estimator (stand-in for src/attacks/pgd/classifier.py TF2Classifier).

Holds the Dense-MLP model, the constraints, the ML scaler and the experiment parameters, and
owns the device attack object (``_native.Pgd``).  ``loss_gradient`` is
classifier.py:107-332 for ``constraints_optim: "sum"``: the gradient, with respect to the
scaled rows, of

    constraints+flip   loss_class - sum(constraints.evaluate(unscale(x), use_tensors=True))
    constraints        -sum(...)
    anything else      loss_class                      ("flip" lands here)

where loss_class is the cross-entropy taken from the logits (d loss / d logit = p - y).
Keras 2.5's probability-clipping path (clip(p, 1e-7, 1 - 1e-7), zero gradient when saturated)
may differ on saturated rows; neither TensorFlow nor ART can be run next to this package, so
the logits form is the engine's definition.
"""
import numpy as np

from ..._native import PGD_LOSS_CONSTRAINTS, PGD_LOSS_FLIP, Pgd

REJECTED_MODES = ("manual", "alternate", "constraints+flip+constraints", "sat", "autopgd")


def check_loss_evaluation(loss_evaluation: str) -> str:
    """The mode strings of the RQ1 / RQ2 sweeps; the reference's other schedules are not
    built."""
    loss_evaluation = "" if loss_evaluation is None else str(loss_evaluation)
    for word in REJECTED_MODES:
        if word in loss_evaluation:
            raise ValueError(f"loss_evaluation {loss_evaluation!r}: the {word!r} schedule is "
                             "not supported (flip, constraints, constraints+flip, "
                             "+adaptive_eps_step, +repair)")
    return loss_evaluation


def loss_flags(loss_evaluation: str) -> int:
    """classifier.py:254-259."""
    loss_evaluation = check_loss_evaluation(loss_evaluation)
    if "constraints+flip" in loss_evaluation:
        return PGD_LOSS_FLIP | PGD_LOSS_CONSTRAINTS
    if "constraints" in loss_evaluation:
        return PGD_LOSS_CONSTRAINTS
    return PGD_LOSS_FLIP


class TF2Classifier:
    def __init__(self, model, constraints, scaler, parameters=None, clip_values=(0.0, 1.0),
                 nb_classes=2, device=0, **_ignored):
        parameters = dict(parameters or {})
        optim = parameters.get("constraints_optim", "sum")
        if optim != "sum":
            raise ValueError(f"constraints_optim {optim!r}: only 'sum' is supported")
        check_loss_evaluation(parameters.get("loss_evaluation", ""))
        if tuple(clip_values) != (0.0, 1.0):
            raise ValueError(f"clip_values {clip_values!r}: the attack clips to (0, 1)")
        self._model = model
        self._constraints = constraints
        self._scaler = scaler
        self._parameters = parameters
        self.clip_values = (0.0, 1.0)
        mlp = model.dense_weights()
        self.nb_classes = int(mlp.weights[-1].shape[1])
        groups, install = constraints.tensor_repair()
        self.device = device
        self.pgd = Pgd(constraints.tensor_program(), mlp.weights, mlp.biases, scaler.scale_,
                       scaler.min_, np.asarray(constraints.get_mutable_mask()).astype(bool),
                       groups, install, tol=getattr(constraints, "tol", 1e-3), device=device)

    @property
    def mutable_mask(self):
        return np.asarray(self._constraints.get_mutable_mask()).astype(bool)

    def _labels(self, y):
        y = np.asarray(y)
        return (np.argmax(y, axis=1) if y.ndim == 2 else y).astype(np.int32)

    def losses_and_gradient(self, x, y, loss_evaluation=None):
        """(gradient (n, D), losses (n, 2 + C)) float32: mv_pgd_grad's two outputs."""
        import torch

        mode = self._parameters.get("loss_evaluation", "") if loss_evaluation is None \
            else loss_evaluation
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x), np.float32)).to(dev)
        yd = torch.from_numpy(np.ascontiguousarray(self._labels(y))).to(dev)
        g = torch.empty_like(xd)
        losses = torch.empty((xd.shape[0], 2 + self.pgd.C), dtype=torch.float32, device=dev)
        self.pgd.grad(xd, yd, loss_flags(mode), g, losses, stream=torch.cuda.current_stream(dev))
        return g.cpu().numpy(), losses.cpu().numpy()

    def loss_gradient(self, x, y, iter_i=0, **_ignored):
        return self.losses_and_gradient(x, y)[0]
