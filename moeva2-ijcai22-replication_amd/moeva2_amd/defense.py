"""Adversarial retraining: the defense loop of src/experiments/lcld/01_train_robust.py
(:208-293 with MoEvA2, :297-397 with C-PGD).

1. candidates: the training rows of class 1 the model gets right at ``threshold`` and that
   satisfy every constraint;
2. attack them (``Moeva2.generate`` or ``PGDTF2.generate``);
3. keep one successful adversarial per candidate
   (``ObjectiveCalculator.get_successful_attacks`` with the reference's arguments);
4. append them to the training set with label 1;
5. train a freshly initialised model of the same architecture on the device.

Not mirrored: shap / important-feature selection, SMOTE and the sampler, AUROC printing and
the intersection of the two adversarial sets (:401-409).
"""
import numpy as np

from .attacks.moeva2.classifier import Classifier
from .attacks.moeva2.objective_calculator import ObjectiveCalculator
from .experiments import training

PGD_LOSS_EVALUATION = "constraints+flip+adaptive_eps_step+repair"


def select_candidates(model, constraints, scaler, x_train, y_train, threshold):
    """01_train_robust.py:208-223: rows of class 1 with predict_proba[:, 1] >= threshold whose
    largest constraint value is <= 0.  Returns (rows, their indices in x_train)."""
    x_train = np.asarray(x_train)
    y = training.class_indices(y_train)
    pred = (model.predict_proba(scaler.transform(x_train))[:, 1] >= threshold).astype(int)
    idx = np.flatnonzero((y == 1) & (pred == y))
    if idx.size:
        ok = np.max(constraints.evaluate(x_train[idx]), axis=1) <= 0
        idx = idx[ok]
    return x_train[idx], idx


def _inverse_transform(scaler, x):
    x = np.array(x, dtype=np.float64, copy=True)
    x -= scaler.min_
    x /= scaler.scale_
    return x


def attack_moeva(model, constraints, scaler, x_candidates, norm, budget, seed, n_pop=200,
                 n_offsprings=100, **kwargs):
    """:238-256 -> (n_candidates, pop_size, D) rows in feature space."""
    from .attacks.moeva2.feature_encoder import get_encoder_from_constraints
    from .attacks.moeva2.moeva2 import Moeva2
    from .attacks.moeva2.utils import results_to_numpy_results

    moeva = Moeva2(model, constraints, problem_class=None, l2_ball_size=0.0, norm=norm,
                   n_gen=budget, n_pop=n_pop, n_offsprings=n_offsprings, scale_objectives=False,
                   save_history=None, seed=seed, n_jobs=1, ml_scaler=scaler, verbose=0, **kwargs)
    return results_to_numpy_results(moeva.generate(x_candidates, 1),
                                    get_encoder_from_constraints(constraints))


def attack_pgd(model, constraints, scaler, x_candidates, norm, budget, eps,
               loss_evaluation=PGD_LOSS_EVALUATION, **kwargs):
    """:337-384 -> (n_candidates, 1, D) rows in feature space.  The rows carry label 1 and the
    attack raises their loss (the reference states the same move as a targeted attack towards
    class 0)."""
    from .attacks.pgd.atk import PGDTF2
    from .attacks.pgd.classifier import TF2Classifier

    est = TF2Classifier(model, constraints, scaler,
                        parameters={"constraints_optim": "sum", "loss_evaluation": loss_evaluation})
    attack = PGDTF2(est, eps=eps - 0.000001, eps_step=0.1, norm=norm, max_iter=int(budget),
                    batch_size=max(int(x_candidates.shape[0]), 1), loss_evaluation=loss_evaluation,
                    **kwargs)
    y = np.ones(x_candidates.shape[0], np.int32)
    x_adv = attack.generate(x=scaler.transform(x_candidates), y=y,
                            mask=constraints.get_mutable_mask())
    return _inverse_transform(scaler, x_adv)[:, np.newaxis, :]


def adversarial_retrain(model, constraints, scaler, x_train, y_train, attack="moeva",
                        threshold=0.5, eps=0.2, norm=2, budget=100, seed=42, epochs=100,
                        batch_size=512, patience=25, **attack_kwargs):
    """One round of adversarial retraining; returns (new_model, info).

    ``x_train`` are feature-space rows, ``y_train`` class indices or one-hot rows; ``scaler``
    has ``transform``, ``scale_`` and ``min_``.  ``info``: candidates, successes, retrain_rows,
    epochs, train_loss, val_loss (and val_accuracy, stopped_early)."""
    if attack not in ("moeva", "pgd"):
        raise ValueError(f"attack {attack!r}: 'moeva' or 'pgd'")
    x_train = np.asarray(x_train, np.float64)
    y = training.class_indices(y_train)
    x_cand, _ = select_candidates(model, constraints, scaler, x_train, y, threshold)
    n_cand = int(x_cand.shape[0])
    if n_cand:
        if attack == "moeva":
            x_gen = attack_moeva(model, constraints, scaler, x_cand, norm, budget, seed,
                                 **attack_kwargs)
        else:
            x_gen = attack_pgd(model, constraints, scaler, x_cand, norm, budget, eps,
                               **attack_kwargs)
        calc = ObjectiveCalculator(Classifier(model), constraints, minimize_class=1,
                                   thresholds={"f1": threshold, "f2": eps},
                                   min_max_scaler=scaler, ml_scaler=scaler, norm=norm)
        x_adv = calc.get_successful_attacks(x_cand, x_gen, preferred_metrics="misclassification",
                                            order="asc", max_inputs=1)
        x_adv = np.asarray(x_adv, np.float64).reshape(-1, x_train.shape[1])
    else:
        x_gen = np.zeros((0, 0, x_train.shape[1]))
        x_adv = np.zeros((0, x_train.shape[1]))
    x_aug = np.concatenate([x_train, x_adv], axis=0)
    y_aug = np.concatenate([y, np.ones(x_adv.shape[0], np.int32)])
    fresh = training.glorot_model(model.dense_weights().dims, seed)
    new_model, fit_info = training.fit(fresh, scaler.transform(x_aug), y_aug, seed=seed,
                                       epochs=epochs, batch_size=batch_size, patience=patience,
                                       return_info=True)
    info = {"candidates": n_cand, "generated_per_candidate": int(x_gen.shape[1]),
            "successes": int(x_adv.shape[0]), "base_rows": int(x_train.shape[0]),
            "retrain_rows": int(x_aug.shape[0])}
    info.update(fit_info)
    return new_model, info
