"""Times the C-PGD kernel (mv_pgd_run) against the same attack written with torch autograd on
the same GPU, at the RQ1 shapes: all LCLD candidates and the 387 botnet states, budget 100 and
1000, mode constraints+flip+adaptive_eps_step, norm 2.  HIP events around each run, warm-up
plus RUNS timed runs, median reported; prints one JSON line per (project, budget).

    python tools/pgd_bench.py [--runs 5] [--torch-runs 1] [--budgets 100 1000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "moeva2-ijcai22-replication_amd"), os.path.join(ROOT, "tests")]

import pgd_torch_ref as ref  # noqa: E402

MODE = "constraints+flip+adaptive_eps_step"
EPS = 0.2 - 1e-6


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def torch_attack(spec, x0, mask, budget):
    """ref.Spec.attack with every tensor on the GPU (labels from the model's prediction)."""
    y = torch.argmax(spec.logits(x0), 1)
    x = x0.clone()
    for i in range(budget):
        g = spec.grad(x, y, MODE)[0]
        eta = float(EPS * (1 / np.float_power(10.0, np.float64(i // (budget // 7) + 1))))
        x = spec.step(x, x0, g, mask, 2, EPS, eta)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--torch-runs", type=int, default=1)
    ap.add_argument("--budgets", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--projects", nargs="+", default=["lcld", "botnet"])
    args = ap.parse_args()
    from moeva2_amd._native import PGD_LOSS_CONSTRAINTS, PGD_LOSS_FLIP
    from moeva2_amd.attacks.moeva2.classifier import load_model
    from moeva2_amd.attacks.pgd.classifier import TF2Classifier
    from moeva2_amd.experiments.united.moeva_run import NpzScaler
    from moeva2_amd.experiments.united.utils import get_constraints_from_str

    dev = torch.device("cuda", 0)
    for project in args.projects:
        feat = os.path.join(ref.RES, "data", project, "features.csv")
        c = get_constraints_from_str(project)(feat, feat.replace("features", "constraints"))
        name = {"lcld": "x_candidates_synthetic.npy", "botnet": "x_candidates_common.npy"}[project]
        x = np.load(os.path.join(ref.RES, "data", project, name), allow_pickle=False)
        scaler = NpzScaler(os.path.join(ref.RES, "models", project, "scaler.npz"))
        est = TF2Classifier(load_model(os.path.join(ref.RES, "models", project, "nn.npz")), c,
                            scaler, parameters={"constraints_optim": "sum"})
        xd = torch.from_numpy(np.clip(scaler.transform(x), 0, 1).astype(np.float32)).to(dev)
        xa = torch.empty_like(xd)
        spec = ref.Spec(project, torch.float32)
        for k in ("W", "b"):
            setattr(spec, k, [t.to(dev) for t in getattr(spec, k)])
        spec.scale, spec.min = spec.scale.to(dev), spec.min.to(dev)
        mask = torch.as_tensor(np.asarray(c.get_mutable_mask()).astype(bool)).to(dev)
        for budget in args.budgets:
            flags = PGD_LOSS_FLIP | PGD_LOSS_CONSTRAINTS
            k_ms, k_all = timed(lambda: est.pgd.run(xd, xa, budget, 2, EPS, 0.1, flags, True),
                                2, max(args.runs, 5))
            out = {"project": project, "rows": int(x.shape[0]), "budget": budget,
                   "kernel_ms_median": k_ms, "kernel_ms": k_all,
                   "kernel_row_iter_per_s": x.shape[0] * budget / (k_ms * 1e-3)}
            if args.torch_runs > 0:
                t_ms, t_all = timed(lambda: torch_attack(spec, xd, mask, budget), 1,
                                    args.torch_runs)
                out.update(torch_ms_median=t_ms, torch_ms=t_all,
                           torch_row_iter_per_s=x.shape[0] * budget / (t_ms * 1e-3),
                           speedup=t_ms / k_ms)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
