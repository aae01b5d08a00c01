"""Times C-PGD on user-defined constraint expressions (MV_OP_EXPR tensor-path columns,
k_pgd<true>) three ways on the same GPU: the dedicated LCLD tensor program, the same program
written as expressions (examples/generic.py lcld_tensor_expressions), and the attack written
with torch autograd (tests/pgd_torch_ref.py).  LCLD candidates tiled to ROWS rows, ITERS
iterations, mode constraints+flip+adaptive_eps_step, norm 2.  HIP events around each run; the
three ways alternate, 2 warm-up rounds and RUNS timed rounds, medians reported; one JSON line.

Gate (exit status 1 when missed): the generic device attack is no slower than torch autograd,
which is what a user without the device derivative would run.  The generic / dedicated ratio
is reported only: the interpreter re-reads the decoded instructions per column per iteration.

    python tools/pgd_expr_speed.py [--rows 4000] [--iters 100] [--runs 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "moeva2-ijcai22-replication_amd"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tools")]

import pgd_torch_ref as ref  # noqa: E402
from pgd_bench import EPS, torch_attack  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    from moeva2_amd._native import PGD_LOSS_CONSTRAINTS, PGD_LOSS_FLIP
    from moeva2_amd.attacks.moeva2.classifier import load_model
    from moeva2_amd.attacks.moeva2.constraints import ExprConstraints
    from moeva2_amd.attacks.pgd.classifier import TF2Classifier
    from moeva2_amd.examples.generic import lcld_expressions, lcld_tensor_expressions
    from moeva2_amd.experiments.united.moeva_run import NpzScaler
    from moeva2_amd.experiments.united.utils import get_constraints_from_str

    dev = torch.device("cuda", 0)
    feat = os.path.join(ref.RES, "data", "lcld", "features.csv")
    cons = feat.replace("features", "constraints")
    dedicated = get_constraints_from_str("lcld")(feat, cons)
    generic = ExprConstraints(feat, cons, lcld_expressions(), lcld_tensor_expressions())
    x = np.load(os.path.join(ref.RES, "data", "lcld", "x_candidates_synthetic.npy"),
                allow_pickle=False)
    x = x[np.arange(args.rows) % x.shape[0]]
    scaler = NpzScaler(os.path.join(ref.RES, "models", "lcld", "scaler.npz"))
    model = load_model(os.path.join(ref.RES, "models", "lcld", "nn.npz"))
    est = {k: TF2Classifier(model, c, scaler, parameters={"constraints_optim": "sum"})
           for k, c in (("dedicated", dedicated), ("generic", generic))}
    xd = torch.from_numpy(np.clip(scaler.transform(x), 0, 1).astype(np.float32)).to(dev)
    out = {k: torch.empty_like(xd) for k in est}
    spec = ref.Spec("lcld", torch.float32)
    for k in ("W", "b"):
        setattr(spec, k, [t.to(dev) for t in getattr(spec, k)])
    spec.scale, spec.min = spec.scale.to(dev), spec.min.to(dev)
    mask = torch.as_tensor(np.asarray(dedicated.get_mutable_mask()).astype(bool)).to(dev)
    flags = PGD_LOSS_FLIP | PGD_LOSS_CONSTRAINTS
    ways = {
        "dedicated": lambda: est["dedicated"].pgd.run(xd, out["dedicated"], args.iters, 2, EPS,
                                                      0.1, flags, True),
        "generic": lambda: est["generic"].pgd.run(xd, out["generic"], args.iters, 2, EPS, 0.1,
                                                  flags, True),
        "torch": lambda: torch_attack(spec, xd, mask, args.iters),
    }
    ms = {k: [] for k in ways}
    for r in range(2 + args.runs):
        for k, fn in ways.items():
            t = event_ms(fn)
            if r >= 2:
                ms[k].append(t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # the two programs share their columns bit for bit, not their gradient arithmetic
    diff = float((out["dedicated"] - out["generic"]).abs().max())
    res = {"rows": args.rows, "iters": args.iters, "ms": ms, "ms_median": med,
           "generic_over_dedicated": med["generic"] / med["dedicated"],
           "torch_over_generic": med["torch"] / med["generic"],
           "max_abs_generic_minus_dedicated": diff,
           "gate_generic_no_slower_than_torch": med["generic"] <= med["torch"]}
    print(json.dumps(res), flush=True)
    return 0 if res["gate_generic_no_slower_than_torch"] else 1


if __name__ == "__main__":
    sys.exit(main())
