"""Subprocess half of tests/test_gpu_row_routes.py::test_plan_overflow_build_bit_exact: one
device attack on a synthetic case with the library MOEVA_MI355X_LIB names (the plan-overflow
build), the final genes / F written to an npz.  argv: out.npz case crossover tmp_dir."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # repo root

import numpy as np  # noqa: E402

import conftest  # noqa: E402,F401  (package path)
import synth_problem as sp  # noqa: E402
from test_gpu_row_routes import run_attack  # noqa: E402


def main():
    out, name, cx, tmp = sys.argv[1:5]
    _, g, F, _ = run_attack(sp.build(name, tmp), cx, hist=0)
    np.savez(out, genes=g, F=F)


if __name__ == "__main__":
    main()
