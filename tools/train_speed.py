"""Speed of training on the device at the reference's LCLD shape (src/experiments/lcld/
model.py): 400 000 x 47 synthetic rows, the 64-32-16-2 model, Adam, batch 512, 10 epochs.

  device  mv_train_steps, one call per epoch with a fresh permutation; host clock around the
          epochs + a device synchronise
  split   the same epochs with mv_train_set_profiling: HIP events around each of the two
          launches of every step (k_train_grad, k_train_adam); the events serialise the
          steps, so only the split is taken from these runs
  torch   the fp32 torch restatement (tests/train_torch_ref.py) on this host, 16 threads, over
          --torch-steps steps (its rate does not depend on the step count)

One warm-up run per way, then --runs timed repeats; medians are reported.  Prints one JSON
line.

    python tools/train_speed.py [--runs 3] [--rows 400000] [--epochs 10]
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
sys.path[:0] = [PKG, os.path.join(ROOT, "tests")]

BATCH = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=int, default=400000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_speed.py measures on the GPU: none visible")
    import train_torch_ref as tref
    from moeva2_amd._native import Trainer
    from moeva2_amd.experiments.lcld.model import create_model

    x, y = tref.blobs(args.rows, 47, seed=0)
    mlp = create_model(47, seed=0).dense_weights()
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    per = (args.rows + BATCH - 1) // BATCH
    rng = np.random.default_rng(0)
    perms = [torch.from_numpy(rng.permutation(args.rows).astype(np.int32)).cuda()
             for _ in range(args.epochs)]

    def device_run(profile):
        tr = Trainer(mlp.weights, mlp.biases)
        tr.set_profiling(profile)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in perms:
            tr.steps(xd, yd, BATCH, per, perm=p)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, tr.kernel_times()

    device_run(False)  # warm-up: code objects, buffers
    secs = [device_run(False)[0] for _ in range(args.runs)]
    splits = [device_run(True)[1] for _ in range(args.runs)]
    grad_us = float(np.median([s["grad_ms"] / s["steps"] for s in splits])) * 1e3
    adam_us = float(np.median([s["adam_ms"] / s["steps"] for s in splits])) * 1e3

    torch.set_num_threads(16)

    def torch_run():
        h = tref.TrainRef(mlp.weights, mlp.biases, torch.float32)
        t0 = time.perf_counter()
        h.steps(x, y, BATCH, args.torch_steps)
        return time.perf_counter() - t0

    torch_run()
    tsecs = [torch_run() for _ in range(args.runs)]
    steps = per * args.epochs
    dev_rate = steps / float(np.median(secs))
    torch_rate = args.torch_steps / float(np.median(tsecs))
    print(json.dumps({
        "workload": "lcld train_model", "rows": args.rows, "batch": BATCH, "epochs": args.epochs,
        "steps": steps, "unit": "steps/s", "device": round(dev_rate, 1),
        "device_runs": [round(steps / s, 1) for s in secs],
        "k_train_grad_us": round(grad_us, 2), "k_train_adam_us": round(adam_us, 2),
        "grad_share": round(grad_us / (grad_us + adam_us), 3),
        "torch_fp32_16_threads": round(torch_rate, 1),
        "torch_runs": [round(args.torch_steps / s, 1) for s in tsecs],
        "device_over_torch": round(dev_rate / torch_rate, 2)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
