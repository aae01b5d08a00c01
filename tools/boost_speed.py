"""Speed of a gradient-boosted classifier at the rq1.lcld.static shape: 64 LCLD states, n_pop 200,
100 offspring, 100 generations, full history, norm 2.  One GradientBoostingClassifier of 100
stages of depth 3, fitted here on perturbed LCLD rows, attacked three ways, one Moeva2.generate
each:

  lds     the fitted model itself, k_boost walking a per-workgroup LDS copy of the nodes
          (mv_get_mlp_kernel 10)
  l2      the same with MV_BOOST_LDS=0: k_boost reading the nodes from global memory (9)
  hosted  the same model behind a predict_proba-only wrapper: every generation decodes on the
          device and calls sklearn's predict_proba on the host (moeva2_amd/hosted.py) -- what
          the engine did for this model before k_boost

One warm-up attack per way, then --runs timed rounds that alternate the ways (host clock around
generate(return_device=True) + a device synchronise); the median is reported, with every run,
as evaluations (rows) per second.  The two device routes compute the same bits, which is
checked.  Prints one JSON line and exits 1 when a device route is slower than hosted.

    python tools/boost_speed.py [--runs 5] [--states 64] [--gens 100]
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
KIND = {"lds": 10, "l2": 9, "hosted": -1}


class NpScaler:
    def __init__(self, path):
        d = np.load(path)
        self.scale_, self.min_ = d["scale_"], d["min_"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--gens", type=int, default=100)
    ap.add_argument("--stages", type=int, default=100)
    ap.add_argument("--depth", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boost_speed.py measures on the GPU: none visible")
    from sklearn.ensemble import GradientBoostingClassifier

    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.examples.lcld.lcld_constraints import LcldConstraints
    from moeva2_amd.models.boost import BoostTables

    feat = os.path.join(RES, "data", "lcld", "features.csv")
    cons = LcldConstraints(feat, feat.replace("features", "constraints"))
    Xall = np.load(os.path.join(RES, "data", "lcld", "x_candidates_synthetic.npy"))
    X = Xall[:args.states]
    sc = NpScaler(os.path.join(RES, "models", "lcld", "scaler.npz"))
    # training rows: the candidates, jittered inside the scaler's range; a label that depends
    # on several features
    rng = np.random.default_rng(0)
    xt = np.repeat(Xall, max(1, 4000 // Xall.shape[0] + 1), axis=0)[:4000]
    xm = xt * sc.scale_ + sc.min_
    xm = np.clip(xm + rng.normal(0.0, 0.05, xm.shape), 0.0, 1.0)
    w = rng.normal(size=xm.shape[1])
    y = ((xm @ w + 0.5 * np.sin(7.0 * xm[:, 0]) + rng.normal(0, 0.2, xm.shape[0]))
         > np.median(xm @ w)).astype(int)
    gb = GradientBoostingClassifier(n_estimators=args.stages, max_depth=args.depth,
                                    random_state=0).fit(xm, y)
    tables = BoostTables.from_sklearn(gb)

    class OnlyProba:
        def predict_proba(self, x):
            return gb.predict_proba(x)

    def make(model):
        return Moeva2(model, cons, ml_scaler=sc, norm=2, n_gen=args.gens, n_pop=N_POP,
                      n_offsprings=N_OFF, save_history="full", seed=42)

    dev = make(gb)
    attacks = {"lds": dev, "l2": dev, "hosted": make(OnlyProba())}
    P = N_POP + 3
    evals = X.shape[0] * (P + (args.gens - 1) * N_OFF)

    def run(k):
        # the route switch is read at every classifier launch
        os.environ["MV_BOOST_LDS"] = "0" if k == "l2" else "1"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = attacks[k].generate(X, 1, return_device=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kind = attacks[k].last_engine.mlp_kernel()
        assert kind == KIND[k], (k, kind)
        return dt, out

    final = {}
    for k in attacks:  # warm-up: code objects, engines, buffers
        _, out = run(k)
        final[k] = out[1].cpu().numpy()
    np.testing.assert_array_equal(final["lds"], final["l2"])
    secs = {k: [] for k in attacks}
    for _ in range(args.runs):
        for k in attacks:
            secs[k].append(run(k)[0])
    os.environ.pop("MV_BOOST_LDS", None)
    rate = {k: evals / float(np.median(v)) for k, v in secs.items()}
    res = {"workload": "rq1.lcld.static", "states": int(X.shape[0]), "generations": args.gens,
           "evaluations": evals, "unit": "evals/s",
           "model": {"stages": args.stages, "trees": tables.n_trees, "nodes": tables.n_nodes,
                     "max_depth": args.depth, "node_bytes": tables.n_nodes * 16},
           "median": {k: round(v) for k, v in rate.items()},
           "runs": {k: [round(evals / s) for s in v] for k, v in secs.items()},
           "lds_over_l2": rate["lds"] / rate["l2"],
           "lds_over_hosted": rate["lds"] / rate["hosted"],
           "l2_over_hosted": rate["l2"] / rate["hosted"],
           # sklearn's exp differs from the engine's in the last bits, so the
           # hosted attack may part ways; the best f1 per state should agree closely
           "mean_best_f1": {k: float(F[:, :, 0].min(axis=1).mean()) for k, F in final.items()}}
    print(json.dumps(res))
    return 0 if min(rate["lds"], rate["l2"]) >= rate["hosted"] else 1


if __name__ == "__main__":
    sys.exit(main())
