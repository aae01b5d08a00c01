"""The MV_OP_EXPR edge programs of tests/expr_edges.py, checked without a GPU: the column
count at the LDS bound is the header's, the constant programs fall on both alignment parities,
and the programs are what tests/test_gpu_expr.py takes them for."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import expr_edges as ee
from moeva2_amd.attacks.moeva2 import expr as E


def test_lds_bound_column_count_is_the_headers(tmp_path):
    """cons_lds_total (csrc/kernels.h) evaluated on the host, as api.cpp build_problem does:
    LDS_BOUND_COLUMNS maximal columns are the last program within 160 KiB."""
    cxx = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cxx):
        pytest.skip("hipcc not found")
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "moeva2-ijcai22-replication_amd", "csrc")
    exe = str(tmp_path / "cons_lds_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", csrc,
                    os.path.join(here, "native", "cons_lds_check.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    n = ee.LDS_BOUND_COLUMNS
    args = []
    for k in (n, n + 1):
        prog = ee.program(ee.bound_columns(k), ee.LDS_BOUND_D)
        assert len(prog.expr_code) == k * E.MAX_WORDS and len(prog.expr_const) == k
        args += [str(k), str(ee.pool_words(prog))]
    r = subprocess.run([exe, str(ee.LDS_BOUND_D)] + args, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    (c0, _, cons0, gen0), (c1, _, cons1, gen1) = [[int(v) for v in line.split()]
                                                 for line in r.stdout.splitlines()]
    assert (c0, c1) == (n, n + 1)
    assert cons0 <= ee.LDS_LIMIT < cons1, (cons0, cons1)
    assert max(gen0, gen1) <= ee.LDS_LIMIT  # the refusal is the constraint program's
    print(f"{n} columns: {cons0} B, {n + 1} columns: {cons1} B, limit {ee.LDS_LIMIT} B")


def test_constant_programs_fall_on_both_parities():
    k = ee.constants()
    for odd in (False, True):
        prog = ee.program(ee.constant_columns(odd), 2)
        assert ee.const_parity(prog) == int(odd)
        np.testing.assert_array_equal(np.asarray(prog.expr_const).view(np.uint64),
                                      k.view(np.uint64))
        ref = E.evaluate_numpy(ee.constant_columns(odd), np.ones((2, 2)), tol=-ee.INF)
        np.testing.assert_array_equal(ref[:, int(odd):].view(np.uint64),
                                      np.tile(k.view(np.uint64), (2, 1)))


def test_sumf_pools():
    cols, pools = ee.sumf_columns()
    assert [len(p) for p in pools[:5]] == list(ee.SUMF_SIZES)
    assert len(set(pools[5])) < len(pools[5]) and len(set(pools[4])) < len(pools[4])
    x = ee.sumf_rows()
    assert (x != np.rint(x)).all(axis=1).any()
    ref = E.evaluate_numpy(cols, x, tol=-ee.INF)
    assert (ref[:, 0].view(np.uint64) == 0).all()  # the empty pool: +0.0
    assert (ref[:3, 6].view(np.uint64) == 0).all()  # 0.0 + -0.0
    assert np.signbit(x[:3, 0]).all()
    for j, p in enumerate(pools):  # left to right from 0.0
        s = np.zeros(x.shape[0])
        for f in p:
            s = s + x[:, f]
        np.testing.assert_array_equal(ref[:, j].view(np.uint64), s.view(np.uint64))


@pytest.mark.parametrize("D", [63, 64, 65, 129])
def test_wide_columns_read_every_trip_and_the_last_feature(D):
    feats = set()
    for e in ee.wide_columns(D):
        code, _, pool = E.compile_expr(e, D)
        words, pc = [int(w) for w in code], 0
        while pc < len(words):
            if words[pc] == E.OPCODES["X"]:
                feats.add(words[pc + 1])
            pc += 1 + E.N_OPERANDS.get(words[pc], 0)
        feats |= set(int(f) for f in pool)
    assert D - 1 in feats and 0 in feats
    assert {f // 64 for f in feats} == set(range((D + 63) // 64))
