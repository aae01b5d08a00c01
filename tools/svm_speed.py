"""Speed of a kernel machine at the rq1.lcld.static shape: 64 LCLD states, n_pop 200, 100
offspring, 100 generations, full history, norm 2.  One RBF SVC (probability=True) fitted here
on perturbed LCLD rows of that width (47 features); the support-vector count it got is printed.
Attacked two ways, one Moeva2.generate each:

  device  the fitted model itself: k_svm inside the device loop (mv_get_mlp_kernel 11)
  hosted  the same model behind a predict_proba-only wrapper: every generation decodes on the
          device and calls sklearn's predict_proba on the host (moeva2_amd/hosted.py) -- what
          the engine did for this model before k_svm

One warm-up attack per way, then --runs timed rounds that alternate the ways (host clock around
generate(return_device=True) + a device synchronise); the median is reported, with every run,
as evaluations (rows) per second.  The kernel alone is timed too: mv_forest_predict on an svm
handle over each of --kernel-rows rows with device events (median of the launches after a
warm-up), and the fp64 rate that follows from 3 * rows * n_vec * D flop (rbf: a subtraction and
one fma per term), against the part's vector fp64 peak.
Prints one JSON line and exits 1 when the device route is slower than hosted.

    python tools/svm_speed.py [--runs 5] [--states 64] [--gens 100] [--train 2000]
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
KIND = {"device": 11, "hosted": -1}
PEAK_FP64_VECTOR = 78.6e12  # MI355X data sheet: vector fp64, FLOP/s


class NpScaler:
    def __init__(self, path):
        d = np.load(path)
        self.scale_, self.min_ = d["scale_"], d["min_"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--states", type=int, default=64)
    ap.add_argument("--gens", type=int, default=100)
    ap.add_argument("--train", type=int, default=2000)
    ap.add_argument("--kernel-rows", default="6400,409600")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("svm_speed.py measures on the GPU: none visible")
    from sklearn.svm import SVC

    from moeva2_amd import _native
    from moeva2_amd.attacks.moeva2.moeva2 import Moeva2
    from moeva2_amd.examples.lcld.lcld_constraints import LcldConstraints
    from moeva2_amd.models.svm import SvmTables

    feat = os.path.join(RES, "data", "lcld", "features.csv")
    cons = LcldConstraints(feat, feat.replace("features", "constraints"))
    Xall = np.load(os.path.join(RES, "data", "lcld", "x_candidates_synthetic.npy"))
    X = Xall[:args.states]
    sc = NpScaler(os.path.join(RES, "models", "lcld", "scaler.npz"))
    # training rows: the candidates, jittered inside the scaler's range; a label that depends
    # on several features
    rng = np.random.default_rng(0)
    xt = np.repeat(Xall, max(1, args.train // Xall.shape[0] + 1), axis=0)[:args.train]
    xm = xt * sc.scale_ + sc.min_
    xm = np.clip(xm + rng.normal(0.0, 0.05, xm.shape), 0.0, 1.0)
    w = rng.normal(size=xm.shape[1])
    y = ((xm @ w + 0.5 * np.sin(7.0 * xm[:, 0]) + rng.normal(0, 0.2, xm.shape[0]))
         > np.median(xm @ w)).astype(int)
    svc = SVC(kernel="rbf", probability=True, random_state=0).fit(xm, y)
    tables = SvmTables.from_sklearn(svc)
    print(f"RBF SVC on {xm.shape[0]} rows of {xm.shape[1]} features: {tables.n_vec} support "
          f"vectors", file=sys.stderr)

    class OnlyProba:
        def predict_proba(self, x):
            return svc.predict_proba(x)

    def make(model):
        return Moeva2(model, cons, ml_scaler=sc, norm=2, n_gen=args.gens, n_pop=N_POP,
                      n_offsprings=N_OFF, save_history="full", seed=42)

    attacks = {"device": make(svc), "hosted": make(OnlyProba())}
    P = N_POP + 3
    evals = X.shape[0] * (P + (args.gens - 1) * N_OFF)

    def run(k):
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
    secs = {k: [] for k in attacks}
    for _ in range(args.runs):
        for k in attacks:
            secs[k].append(run(k)[0])
    rate = {k: evals / float(np.median(v)) for k, v in secs.items()}

    # the kernel alone: one launch over the rows of one generation, and over enough rows to
    # fill the part (one lane per row: 6,400 rows are 100 waves on 1,024 SIMDs)
    h = _native.Svm(tables)
    kernel = []
    for n in [int(v) for v in args.kernel_rows.split(",")]:
        xd = torch.as_tensor(rng.uniform(0.0, 1.0, (n, tables.n_features)), device="cuda")
        out = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        h.predict(xd, out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(args.runs, 5)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            h.predict(xd, out)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        kernel_ms = float(np.median(ms))
        # rbf: a subtraction and one fma (two flop) per term
        flop = 3.0 * n * tables.n_vec * tables.n_features
        kernel.append({"rows": n, "ms_per_launch": kernel_ms, "ms_runs": [round(m, 4) for m in ms],
                       "fp64_flop": flop, "fp64_flop_per_s": flop / (kernel_ms * 1e-3),
                       "vector_fp64_peak": PEAK_FP64_VECTOR,
                       "fraction_of_peak": flop / (kernel_ms * 1e-3) / PEAK_FP64_VECTOR})
    res = {"workload": "rq1.lcld.static", "states": int(X.shape[0]), "generations": args.gens,
           "evaluations": evals, "unit": "evals/s",
           "model": {"kernel": "rbf", "train_rows": int(xm.shape[0]),
                     "features": tables.n_features, "support_vectors": tables.n_vec,
                     "gamma": tables.gamma},
           "median": {k: round(v) for k, v in rate.items()},
           "runs": {k: [round(evals / s) for s in v] for k, v in secs.items()},
           "device_over_hosted": rate["device"] / rate["hosted"],
           "kernel": kernel,
           # sklearn's sums and exp differ from the engine's in the last bits, so
           # the hosted attack may part ways; the best f1 per state should agree closely
           "mean_best_f1": {k: float(F[:, :, 0].min(axis=1).mean()) for k, F in final.items()}}
    print(json.dumps(res))
    return 0 if rate["device"] >= rate["hosted"] else 1


if __name__ == "__main__":
    sys.exit(main())
