"""Speed of user-defined constraint expressions (MV_OP_EXPR) at the rq1.lcld.static shape: 64
LCLD states, n_pop 200, 100 offspring, 100 generations, full history, norm 2.  Three ways to
state the same ten LCLD constraints, one Moeva2.generate each:

  dedicated  the shipped LcldConstraints (dedicated op codes: k_narrow)
  generic    ExprConstraints(lcld_expressions()): the interpreter, k_gen + k_consx
  hosted     a foreign subclass whose evaluate is evaluate_numpy: every generation decodes on
             the device and evaluates the constraints on the host (moeva2_amd/hosted.py)

One warm-up attack per way, then --runs timed rounds that alternate the three ways (host
clock around generate(return_device=True) + a device synchronise); the median is reported,
with every run, as evaluations (rows) per second.  Prints one JSON line and exits 1 when
generic < hosted.

    python tools/expr_speed.py [--runs 5] [--states 64] [--gens 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moeva2-ijcai22-replication_amd")
sys.path[:0] = [PKG]

RES = os.path.join(PKG, "resources")
N_POP, N_OFF = 200, 100


class NpScaler:
    def __init__(self, path):
        d = np.load(path)
        self.scale_, self.min_ = d["scale_"], d["min_"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--gens", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("expr_speed.py measures on the GPU: none visible")
    from moeva2_amd.attacks.moeva2.constraints import ExprConstraints
    from moeva2_amd.attacks.moeva2.expr import evaluate_numpy
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.examples.generic import lcld_expressions
    from moeva2_amd.examples.lcld.lcld_constraints import LcldConstraints

    feat = os.path.join(RES, "data", "lcld", "features.csv")
    cons = feat.replace("features", "constraints")
    exprs = lcld_expressions()

    class Foreign(LcldConstraints):
        """A class the engine cannot compile: its numpy evaluate runs on the host."""

        def device_program(self):
            raise NotImplementedError

        def evaluate(self, x, use_tensors=False):
            return evaluate_numpy(exprs, np.atleast_2d(x), tol=self.tol)

    ways = {"dedicated": LcldConstraints(feat, cons),
            "generic": ExprConstraints(feat, cons, exprs),
            "hosted": Foreign(feat, cons)}
    X = np.load(os.path.join(RES, "data", "lcld", "x_candidates_synthetic.npy"))[:args.states]
    sc = NpScaler(os.path.join(RES, "models", "lcld", "scaler.npz"))
    attacks = {k: Moeva2(os.path.join(RES, "models", "lcld", "nn.npz"), c, ml_scaler=sc, norm=2,
                         n_gen=args.gens, n_pop=N_POP, n_offsprings=N_OFF, save_history="full",
                         seed=42)
               for k, c in ways.items()}
    P = N_POP + 3
    evals = X.shape[0] * (P + (args.gens - 1) * N_OFF)

    def run(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = attacks[k].generate(X, 1, return_device=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    final = {}
    for k in attacks:  # warm-up: code objects, engines, buffers
        _, out = run(k)
        final[k] = out[1].cpu().numpy()
    secs = {k: [] for k in attacks}
    for _ in range(args.runs):
        for k in attacks:
            secs[k].append(run(k)[0])
    rate = {k: evals / float(np.median(v)) for k, v in secs.items()}
    res = {"workload": "rq1.lcld.static", "states": int(X.shape[0]), "generations": args.gens,
           "evaluations": evals, "unit": "evals/s",
           "median": {k: round(v) for k, v in rate.items()},
           "runs": {k: [round(evals / s) for s in v] for k, v in secs.items()},
           "generic_over_hosted": rate["generic"] / rate["hosted"],
           "generic_over_dedicated": rate["generic"] / rate["dedicated"],
           # the same attack three ways: best f1 per state should agree closely (the columns
           # are the same values; only f3's summation order differs between the ways)
           "mean_best_f1": {k: float(F[:, :, 0].min(axis=1).mean()) for k, F in final.items()}}
    print(json.dumps(res))
    return 0 if rate["generic"] >= rate["hosted"] else 1


if __name__ == "__main__":
    sys.exit(main())
