"""C-PGD experiment driver (mirror of src/experiments/united/01_pgd_united.py:29-215).

Same configuration keys, same outputs under ``config["dirs"]["results"]``, with
``mid = f"{attack_name}_{loss_evaluation}"``:

  x_attacks_{mid}_{hash}.npy     (n, 1, D) adversarial rows in ML feature space
  success_rate_{mid}_{hash}.csv  o1..o7 of ObjectiveCalculator.success_rate_3d_df
  metrics_{mid}_{hash}.json      {objectives, time, config, config_hash}
  config_{mid}_{hash}.yaml

and the run is skipped when the metrics file exists.  No comet logging and no SAT stage;
``save_history`` other than none is rejected (the loop never leaves the device).

The reference's integer floor / ceil block (:130-137) assigns into a fancy-indexed copy
(``x_attacks[:, mask_int][...] = ...``) and therefore changes nothing; the observable
behaviour is mirrored: the attack rows are NOT rounded.
"""
import json
import os
import time
import warnings
from pathlib import Path

import numpy as np

from ...attacks.moeva2.classifier import Classifier, load_model
from ...attacks.moeva2.objective_calculator import ObjectiveCalculator
from ...attacks.pgd.atk import PGDTF2
from ...attacks.pgd.classifier import TF2Classifier, check_loss_evaluation
from ...config_parser.config_parser import get_config, get_dict_hash, save_config
from .moeva_run import _constraints, filter_initial_states, load_scaler, resolve_path


def mid_fix(config) -> str:
    return f"{config['attack_name']}_{config['loss_evaluation']}"


def output_paths(config) -> dict:
    out_dir, h, mid = config["dirs"]["results"], get_dict_hash(config), mid_fix(config)
    return {"x_attacks": f"{out_dir}/x_attacks_{mid}_{h}.npy",
            "success_rate": f"{out_dir}/success_rate_{mid}_{h}.csv",
            "metrics": f"{out_dir}/metrics_{mid}_{h}.json",
            "config": f"{out_dir}/config_{mid}_{h}.yaml"}


def inverse_transform(scaler, x):
    x = np.array(x, dtype=np.float64, copy=True)
    x -= scaler.min_
    x /= scaler.scale_
    return x


def make_attack(config, constraints, model, scaler):
    """01_pgd_united.py:85-123."""
    est = TF2Classifier(model, constraints, scaler, parameters=config)
    return PGDTF2(est, eps=config["eps"] - 0.000001, eps_step=0.1, norm=config.get("norm"),
                  max_iter=int(config.get("budget")), num_random_init=config.get("nb_random", 0),
                  batch_size=1 << 30, loss_evaluation=config.get("loss_evaluation"))


def run(config, verbose=True, attack_factory=make_attack):
    """One configuration dict; returns the metrics dict (None when skipped)."""
    warnings.simplefilter(action="ignore", category=FutureWarning)
    check_loss_evaluation(config.get("loss_evaluation"))
    if config.get("save_history") not in (None, "", "none", False):
        raise ValueError(f"save_history {config.get('save_history')!r}: the C-PGD loop keeps no "
                         "history (use none)")
    if config.get("constraints_optim", "sum") != "sum":
        raise ValueError(f"constraints_optim {config.get('constraints_optim')!r}: only 'sum'")
    paths_out = output_paths(config)
    config_hash = get_dict_hash(config)
    if os.path.exists(paths_out["metrics"]):
        print(f"Configuration with hash {config_hash} already executed. Skipping")
        return None
    out_dir = config["dirs"]["results"]
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    if verbose:
        print(config)
    paths = config["paths"]
    constraints = _constraints(config["project_name"], paths["features"], paths["constraints"],
                               paths.get("important_features"))
    x_initial = np.load(resolve_path(paths["x_candidates"]), allow_pickle=False)
    x_initial = filter_initial_states(x_initial, config["initial_state_offset"],
                                      config["n_initial_state"])
    model = load_model(resolve_path(paths["model"]))
    scaler = load_scaler(paths["ml_scaler"])
    constraints.check_constraints_error(x_initial)

    start_time = time.time()
    attack = attack_factory(config, constraints, model, scaler)
    x_attacks = inverse_transform(scaler, attack.generate(x=scaler.transform(x_initial),
                                                          mask=constraints.get_mutable_mask()))
    consumed_time = time.time() - start_time
    if x_attacks.ndim == 2:
        x_attacks = x_attacks[:, np.newaxis, :]

    thresholds = {"f1": config["misclassification_threshold"], "f2": config["eps"]}
    calc = ObjectiveCalculator(Classifier(model), constraints, minimize_class=1,
                               thresholds=thresholds, min_max_scaler=scaler, ml_scaler=scaler,
                               norm=config["norm"])
    df = calc.success_rate_3d_df(x_initial, x_attacks)
    if verbose:
        print(df)
    np.save(paths_out["x_attacks"], x_attacks)
    metrics = {"objectives": df.to_dict(orient="records")[0], "time": consumed_time,
               "config": config, "config_hash": config_hash}
    df.to_csv(paths_out["success_rate"], index=False)
    with open(paths_out["metrics"], "w") as f:
        json.dump(metrics, f)
    save_config(f"{out_dir}/config_{mid_fix(config)}_", config)
    return metrics


def main(argv=None):
    t0 = time.time()
    out = run(get_config(argv))
    print(f"func:'run' took: {time.time() - t0:2.4f} sec")
    return out


if __name__ == "__main__":
    main()
