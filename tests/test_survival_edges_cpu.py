"""tests/survival_cases.py on the oracle alone: every case takes the branches it was built for
(its witness), its survivors are distinct, and the parametrisation covers what it claims (the
sweep's residues, both values of surv_offsets' alias on neighbouring N).  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import survival_cases as sc


@pytest.mark.parametrize("name", sc.ALL_CASES)
def test_case_stays_on_its_branch(name):
    case, out = sc.oracle_run(name)
    assert len(case.F) >= 2 and case.F[0].shape[0] >= 3
    for F in case.F:  # states of different data
        assert not np.array_equal(F[0], F[1]) and not np.array_equal(F[1], F[2])
    sc.check_witness(case, out)
    for row in out:
        for r, _snap, _w in row:
            assert len(r.survivors) == case.n_survive
            assert len(set(r.survivors.tolist())) == case.n_survive


def test_branch_families_are_all_present():
    """Across the branch cases every nadir outcome, both clamps on and off, and every
    association route occurs at every N."""
    for N in sc.BRANCH_N:
        ws = [w for n in sc.BRANCH_CASES if n.endswith(f"-N{N}")
              for row in sc.oracle_run(n)[1] for _r, _s, w in row]
        assert {w["nadir"] for w in ws} == {"singular", "notclose", "small", "plane"}
        for key in ("clampworst", "wfront", "den0", "niching"):
            assert {w[key] for w in ws} == {False, True}, key
        for key in ("dotsmall", "clamp", "at_ideal", "nonfinite", "ovf", "ovf5"):
            assert min(w[key] for w in ws) == 0 and max(w[key] for w in ws) > 0, key


def test_r_edges_cover_the_sweep_residues():
    res = [sc.sweep_residues(R) for R in sc.R_EDGES]
    for par in ("even", "odd"):
        assert {a for p, a, _ in res if p == par} == {0, 1, 2, 3}, par
    assert {c for _, _, c in res} == {0, 1, 2, 3}
    assert {1, 8, 61, 62, 63, 64, 65, sc.SURV_RMAX} <= set(sc.R_EDGES)
    for R in sc.R_EDGES:
        assert sc.oracle_run(sc.r_edge_id(R))[0].R == R


def test_alias_in_the_case_ids_is_the_headers(tmp_path):
    """surv_offsets evaluated on the host for every (N, R) of the N edges: the ids carry its
    alias, and both values occur on neighbouring N at each R."""
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("hipcc not found")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "moeva2-ijcai22-replication_amd", "csrc")
    exe = str(tmp_path / "surv_offsets_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-I", csrc,
                    os.path.join(here, "native", "surv_offsets_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    pairs = [(N, R) for R in (20, 200) for N in sc.N_EDGES] + [(1024, 640)]
    r = subprocess.run([exe] + [str(v) for p in pairs for v in p], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in r.stdout.splitlines():
        N, R, alias, total = (int(v) for v in line.split())
        got[(N, R)] = (alias, total)
    assert set(got) == set(pairs)
    for (N, R), (alias, total) in got.items():
        assert alias == sc.alias_of(N, R), (N, R)
        assert sc.n_edge_id(N, R) in sc.CASES
        assert total <= 160 * 1024 or (N, R) == (1024, 640), (N, R, total)
    for R in (20, 200):
        flips = [(a, b) for a, b in zip(sc.N_EDGES, sc.N_EDGES[1:])
                 if b == a + 1 and got[(a, R)][0] != got[(b, R)][0]]
        assert flips, R
