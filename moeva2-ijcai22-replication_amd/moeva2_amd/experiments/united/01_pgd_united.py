"""``python -m moeva2_amd.experiments.united.01_pgd_united -c config/pgd.yaml -c <project>.yaml
-p budget=100 -p eps=0.2 -p loss_evaluation=constraints+flip`` -- same command line as
src/experiments/united/01_pgd_united.py (see pgd_run.py)."""
from moeva2_amd.experiments.united.pgd_run import main

if __name__ == "__main__":
    main()
