"""Subprocess half of tests/test_gpu_mlp_fallback.py for the cases that reach k_mlp only under
development switches (the parent sets them in this process's environment): the kernel kind,
mv_evaluate's outputs and one attack's population and history, written to an npz.
argv: out.npz case tmp_dir."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # repo root

import numpy as np  # noqa: E402

import conftest  # noqa: E402,F401  (package path)
import synth_problem as sp  # noqa: E402
from test_gpu_mlp_fallback import ROWS, run_device  # noqa: E402


def main():
    out, name, tmp = sys.argv[1:4]
    sy = sp.build(name, tmp)
    kind, Fs, att = run_device(sy, sy.case.mlp_v1)
    g, F, h, stored = att["two_point"]
    np.savez(out, mlp_kernel=kind, g=g, F=F, h=h, stored=stored,
             **{f"F{n}": Fs[n] for n in ROWS})


if __name__ == "__main__":
    from moeva2_amd._native import NativeError

    try:
        main()
    except NativeError as e:
        if "error 2" in str(e):  # MV_ERR_HIP: the parent ends the session on exit status 3
            print(e, file=sys.stderr)
            sys.exit(3)
        raise
