"""Speed of a random-forest classifier at the rq1.lcld.static shape: 64 LCLD states, n_pop 200,
100 offspring, 100 generations, full history, norm 2.  One 100-tree forest of depth <= 12,
fitted here on perturbed LCLD rows, attacked two ways, one Moeva2.generate each:

  device  the fitted forest itself: its trees run inside the device loop (k_forest)
  hosted  the same forest behind a predict_proba-only wrapper: every generation decodes on the
          device and calls sklearn's predict_proba (n_jobs 1) on the host (moeva2_amd/hosted.py)

One warm-up attack per way, then --runs timed rounds that alternate the two ways (host clock
around generate(return_device=True) + a device synchronise); the median is reported, with
every run, as evaluations (rows) per second.  Prints one JSON line and exits 1 when
device < hosted.

    python tools/forest_speed.py [--runs 5] [--states 64] [--gens 100]
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
    ap.add_argument("--trees", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("forest_speed.py measures on the GPU: none visible")
    from sklearn.ensemble import RandomForestClassifier

    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.examples.lcld.lcld_constraints import LcldConstraints
    from moeva2_amd.models.forest import ForestTables

    feat = os.path.join(RES, "data", "lcld", "features.csv")
    cons = LcldConstraints(feat, feat.replace("features", "constraints"))
    Xall = np.load(os.path.join(RES, "data", "lcld", "x_candidates_synthetic.npy"))
    X = Xall[:args.states]
    sc = NpScaler(os.path.join(RES, "models", "lcld", "scaler.npz"))
    # training rows: the candidates, jittered inside the scaler's range; a label that depends
    # on several features so the trees grow to the depth limit
    rng = np.random.default_rng(0)
    xt = np.repeat(Xall, max(1, 4000 // Xall.shape[0] + 1), axis=0)[:4000]
    xm = xt * sc.scale_ + sc.min_
    xm = np.clip(xm + rng.normal(0.0, 0.05, xm.shape), 0.0, 1.0)
    w = rng.normal(size=xm.shape[1])
    y = ((xm @ w + 0.5 * np.sin(7.0 * xm[:, 0]) + rng.normal(0, 0.2, xm.shape[0]))
         > np.median(xm @ w)).astype(int)
    forest = RandomForestClassifier(n_estimators=args.trees, max_depth=12, random_state=0,
                                    n_jobs=1).fit(xm, y)
    tables = ForestTables.from_sklearn(forest)

    class OnlyProba:
        def predict_proba(self, x):
            return forest.predict_proba(x)

    attacks = {k: Moeva2(m, cons, ml_scaler=sc, norm=2, n_gen=args.gens, n_pop=N_POP,
                         n_offsprings=N_OFF, save_history="full", seed=42)
               for k, m in (("device", forest), ("hosted", OnlyProba()))}
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
    assert attacks["device"].last_engine.mlp_kernel() == 8  # k_forest
    secs = {k: [] for k in attacks}
    for _ in range(args.runs):
        for k in attacks:
            secs[k].append(run(k)[0])
    rate = {k: evals / float(np.median(v)) for k, v in secs.items()}
    res = {"workload": "rq1.lcld.static", "states": int(X.shape[0]), "generations": args.gens,
           "evaluations": evals, "unit": "evals/s",
           "forest": {"trees": tables.n_trees, "nodes": tables.n_nodes,
                      "max_depth": int(max(e.tree_.max_depth for e in forest.estimators_))},
           "median": {k: round(v) for k, v in rate.items()},
           "runs": {k: [round(evals / s) for s in v] for k, v in secs.items()},
           "device_over_hosted": rate["device"] / rate["hosted"],
           # sklearn's leaf rows differ from the restatement's in the last bit,
           # so the two attacks may part ways; their best f1 per state should agree closely
           "mean_best_f1": {k: float(F[:, :, 0].min(axis=1).mean()) for k, F in final.items()}}
    print(json.dumps(res))
    return 0 if rate["device"] >= rate["hosted"] else 1


if __name__ == "__main__":
    sys.exit(main())
