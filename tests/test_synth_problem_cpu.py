"""The synthetic problems of tests/synth_problem.py, checked without a GPU: the product's
encoder lays the genes out as the oracle does, the inputs make the constraints bite without
saturating, the compact cases fix the intended genes, and every case's shape and expected
kernels are the ones a line of the route table (tests/test_routes_cpu.py) pins.  For the cases
with MV_OP_EXPR columns: the restated columns equal ``eval_ops`` bit for bit."""
import re

import numpy as np
import pytest

import synth_problem as sp
from oracle import device_order as do
from oracle import moeva_oracle as mo
from test_routes_cpu import EXPECTED

NAMES = [c.name for c in sp.CASES]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sp.build(name, d)
        return cache[name]

    return get


@pytest.mark.parametrize("name", NAMES)
def test_layout_matches_oracle(built, name):
    from moeva2_amd.attacks.moeva2.feature_encoder import get_encoder_from_constraints
    from moeva2_amd.problem import build_device_program

    sy, case = built(name), sp.CASES_BY_NAME[name]
    lay = sy.lay
    assert (lay.V, int(lay.mutable_mask.sum())) == (case.V, case.Dm)
    assert [len(m) for m in lay.ohe_masks] == list(case.ohe)
    prog = build_device_program(sy.constraints)
    np.testing.assert_array_equal(prog.op_code, sy.codes)
    assert (prog.V, prog.C, prog.D) == (case.V, case.C, sy.D)
    mut = np.where(lay.mutable_mask)[0]
    np.testing.assert_array_equal(prog.mut_feats, mut)
    n = int(lay.no_ohe_mask.sum())
    np.testing.assert_array_equal(prog.gene_feat[:n], mut[lay.no_ohe_mask])
    types = mo.genetic_types(lay)
    np.testing.assert_array_equal(prog.gene_kind[:n], [0 if t == "real" else 1 for t in types[:n]])
    np.testing.assert_array_equal(prog.gene_kind[n:], 2)
    np.testing.assert_array_equal(prog.gene_feat[n:], np.arange(len(case.ohe)))
    np.testing.assert_array_equal(np.diff(prog.ohe_offsets), list(case.ohe))
    if case.ohe:
        np.testing.assert_array_equal(prog.ohe_feats, np.concatenate([mut[m] for m in lay.ohe_masks]))
        # the first group opens the mutable features, the last one closes them
        assert lay.ohe_masks[0][0] == 0 and lay.ohe_masks[-1][-1] == case.Dm - 1 or len(case.ohe) == 1
    xl, xu = sy.bounds()
    dyn = 0
    for s, prob in enumerate(sy.probs):
        enc = get_encoder_from_constraints(sy.constraints, sy.X[s])
        np.testing.assert_array_equal(xl[s], prob.xl)
        np.testing.assert_array_equal(xu[s], prob.xu)
        gl, gu = mo.genetic_bounds(lay, prob.xl, prob.xu)
        el, eu = enc.get_min_max_genetic()
        np.testing.assert_array_equal(el, gl)
        np.testing.assert_array_equal(eu, gu)
        np.testing.assert_array_equal(enc.get_type_mask_genetic(), types)
        g0 = mo.ml_to_genetic(lay, sy.X[s][None])[0]
        np.testing.assert_array_equal(enc.ml_to_genetic(sy.X[s][None])[0], g0)
        isi = types != "real"
        assert (np.rint(g0[isi]) == g0[isi]).all() and (g0 >= gl).all() and (g0 <= gu).all()
        for m in lay.ohe_masks:  # a valid one-hot group
            v = sy.X[s][mut[m]]
            assert v.sum() == 1.0 and set(v) <= {0.0, 1.0}
        dyn += int((gl[:n] == g0[:n]).sum())
        for nm, a, _ in sy.ops:  # ratio denominators >= 1 inside the bounds (or immutable, != 0)
            for f in {"RATIO_SAFE": a[1:2], "ABS_RATIO": a[2:3], "RATIO_MASKED": a[2:3]}.get(nm, ()):
                assert prob.xl[f] >= 1.0 if lay.mutable_mask[f] else sy.X[s][f] != 0.0
    assert dyn > 0 or case.n_plain < 4  # some lower bounds are the input's value
    assert all(np.abs(v - 1).min() > 0.04 for v in sy.ml[:1]) and (sy.ml[1] != 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_constraints_bite_without_saturating(built, name):
    """On the oracle alone, over the rows the GPU case evaluates: at least 10 % of the rows
    have f3 > 0, at least 10 % have f3 == 0, at least half of the columns are positive on
    some row -- and the engine-order restatement agrees with the plain oracle."""
    sy = built(name)
    genes, inf_rows = sy.eval_genes(np.random.default_rng(sp.case_seed(name) + 1))
    f3, pos = [], np.zeros(sy.case.C, bool)
    for b, prob in enumerate(sy.probs):
        F, G = mo.evaluate(prob, genes[b], return_g=True)
        assert np.isfinite(np.delete(F, inf_rows, axis=0)[:, :2]).all() and not np.isnan(F[:, 2]).any()
        Fd = do.evaluate_device_order(prob, genes[b], sy.codes)
        fin = np.setdiff1d(np.arange(F.shape[0]), inf_rows)
        np.testing.assert_allclose(Fd[fin, 0], F[fin, 0], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(Fd[fin, 1:], F[fin, 1:], rtol=1e-12, atol=1e-15)
        f3.append(F[:, 2])
        pos |= (G > 0).any(axis=0)
    f3 = np.concatenate(f3)
    print(name, "f3 > 0:", (f3 > 0).mean(), "f3 == 0:", (f3 == 0).mean(), "columns:", pos.mean())
    assert (f3 > 0).mean() >= 0.10
    assert (f3 == 0).mean() >= 0.10
    assert pos.mean() >= 0.5


def _intended_fixed(case, sy):
    fixed = np.zeros(sy.D, bool)
    if case.fixed is not None:
        for g in range(case.n_plain):
            if len(tuple(case.fixed(g))) == sp.B:
                fixed[sy.plain_feat[g]] = True
    return fixed


@pytest.mark.parametrize("name", NAMES)
def test_compact_masks(built, name):
    sy, case = built(name), sp.CASES_BY_NAME[name]
    fixed = do.compact_fixed(sy.lay, sy.probs)
    np.testing.assert_array_equal(fixed, _intended_fixed(case, sy))
    assert fixed.sum() == sp.N_FIXED.get(name, 0)
    if name in ("k_mixed", "xk_mixed"):  # gene 7: fixed in states 0 and 1 only, so it is stored
        fx = [do.compact_fixed(sy.lay, [p])[sy.plain_feat[7]] for p in sy.probs]
        assert fx == [True, True, False] and not fixed[sy.plain_feat[7]]


_ROW = {0: "k_gen+k_cons", 1: "k_narrow", 2: "k_genc"}
_MLP = {1: "k_mlp2(genes)", 2: "k_mlp2", 6: "k_mlpr(genes)", 7: "k_mlpr"}
_LINE = re.compile(r"row synth (\S+) V(\d+) Dm4 (\d+) C(\d+) i(\d) f(\d) sd(\d+) c(\d) s(\d) x(\d)"
                   r"\s+kind=(\d) nt=(\d+) ident=(\d) sbx=(\d) slim=(\d) cons=(\d) nv=(\d+) "
                   r"full=(\d) need_plan=\d plan_missing=\d mlp=(-?\d)$")


def _route_lines():
    out = {}
    for line in EXPECTED.splitlines():
        m = _LINE.match(line)
        if m:
            out[m.group(1)] = [int(v) for v in m.groups()[1:]]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_route_table_pins_the_case(built, name):
    """The route table's line of this case was computed for the shape the builder makes, and
    gives the kernels the GPU case asserts (tests/test_gpu_row_routes.py)."""
    sy, case = built(name), sp.CASES_BY_NAME[name]
    lines = _route_lines()
    sh = sp.engine_shape(case, sy, do.compact_fixed(sy.lay, sy.probs))
    for key, sbx in [(name, 0)] + ([(name + "/sbx", 1)] if case.sbx else []):
        v = lines[key]
        assert v[:9] == [sh["V"], sh["Dm4"], sh["C"], sh["ident"], sh["full_ops"], sh["sd"],
                         sh["compact"], sh["slim"], sbx], (key, v, sh)
        kind, mlp = v[9], v[-1]
        assert _ROW[kind] == ((case.row_sbx or case.row) if sbx else case.row)
        assert _MLP[mlp] == case.mlp
    assert not [k for k in lines if k.split("/")[0] not in sp.CASES_BY_NAME]


def test_every_instance_family_has_a_line():
    """k_narrow NV 8/16/32 x FULL; k_gen / k_cons NT 1/2/4/8/16 x IDENT; k_genc NT 4..8 and 16;
    SLIM false; SBX per family; the five compact patterns."""
    L = list(_route_lines().values())
    K, NT, ID, SBX, SLIM, CONS, NV, FULL = 9, 10, 11, 12, 13, 14, 15, 16
    for nv in (8, 16, 32):
        for full in (0, 1):
            assert any(v[K] == 1 and v[NV] == nv and v[FULL] == full for v in L), (nv, full)
    for ident, nts in ((1, (1, 2)), (0, (1, 2, 4, 8, 16))):
        for nt in nts:
            assert any(v[K] == 0 and v[NT] == nt and v[ID] == ident for v in L), (ident, nt)
    assert any(v[K] == 0 and v[CONS] == 2 and v[NT] == 8 for v in L)
    for nt in (4, 5, 6, 7, 8, 16):
        assert any(v[K] == 2 and v[NT] == nt and v[SLIM] == 1 for v in L), nt
    assert any(v[K] == 2 and v[SLIM] == 0 for v in L)
    assert any(v[K] == 2 and v[SBX] == 1 for v in L)
    assert any(v[K] == 0 and v[SBX] == 1 and v[ID] == 1 and v[0] <= 8 for v in L)
    assert any(v[K] == 0 and v[SBX] == 1 and v[ID] == 0 for v in L)
    assert sum(v[6] for v in L) == len(sp.COMPACT) == 9
    for ident in (0, 1):  # k_consx<IDENT, NT>: the ten instances
        for nt in (1, 2, 4, 8, 16):
            assert any(v[K] == 0 and v[CONS] == 3 and v[NT] == nt and v[ID] == ident for v in L), \
                (ident, nt)
    assert any(v[CONS] == 3 and v[SBX] == 1 and v[ID] == ident for ident in (0, 1) for v in L)
    assert sum(v[CONS] == 3 and v[6] for v in L) == 4  # ... and with a compact gene set


# ------------------------------------------------------------------ MV_OP_EXPR cases
# (caller pool entries + code words) & 1 per case: odd -> the engine pads one word in front of
# the constants it appends to the index pool.  Both sides occur.
POOL_PARITY = {"x64": 0, "x65": 1, "x128": 0, "x129": 0, "x256": 0, "x257": 1, "x512": 0,
               "x513": 0, "x1024": 0, "x300c": 1, "xo32d": 1, "xo100": 1, "xo300f": 1, "xo520": 0,
               "xn8f": 0, "xk_last": 1, "xk_odd": 1, "xk_few": 1, "xk_mixed": 1}


def test_expr_cases_cover_both_pool_parities():
    assert set(POOL_PARITY) == set(sp.EXPR) and set(POOL_PARITY.values()) == {0, 1}
    assert [n for n in sp.EXPR if sp.CASES_BY_NAME[n].expr == "all"]
    assert [n for n in sp.EXPR if sp.CASES_BY_NAME[n].expr == "mixed"]


@pytest.mark.parametrize("name", sp.EXPR)
def test_restatement_equals_the_ops_bit_for_bit(built, name):
    """evaluate_numpy of the restated columns against eval_ops -- which stays the statement
    of the values -- on the rows the GPU case evaluates: the same bits, NaN in the same places
    (the LCLD_INSTALL column, np.power on both sides, at 1e-14).  And the program's shape:
    which columns are EXPR, that ABS_SUMDIFF stays dedicated in the mixed mode, and the parity
    of the words in front of the constants."""
    from moeva2_amd.attacks.moeva2 import expr as E

    sy, case = built(name), sp.CASES_BY_NAME[name]
    cols = sy.expressions()
    idx = sorted(cols)
    names = [sy.ops[c][0] for c in range(case.C)]
    if case.expr == "all":
        assert idx == list(range(case.C))
    else:
        assert idx == [c for c in range(case.C) if c % 3 == 2 and names[c] != "ABS_SUMDIFF"]
        assert {names[c] for c in idx} >= {"DIFF", "RATIO_SAFE"}
        assert {names[c] for c in range(case.C) if c not in cols} >= {"DIFF", "RATIO_SAFE"}
    assert (sy.codes[idx] == 16).all() and (np.delete(sy.codes, idx) != 16).all()
    prog = sy.constraints.device_program()
    np.testing.assert_array_equal(prog.arrays()[0], sy.codes)
    assert sy.pool_parity() == POOL_PARITY[name]
    assert sum(n == "ABS_SUMDIFF" and c not in cols for c, n in enumerate(names)) == \
        (0 if case.expr == "all" else len(case.sumdiff))
    genes, _ = sy.eval_genes(np.random.default_rng(sp.case_seed(name) + 1))
    exact = [c for c in idx if names[c] != "LCLD_INSTALL"]
    install = [c for c in idx if names[c] == "LCLD_INSTALL"]
    assert len(install) == int(case.install and case.expr == "all")
    seen_nan = seen_pos = False
    for b, prob in enumerate(sy.probs):
        x = mo.genetic_to_ml(sy.lay, genes[b], prob.x_init)
        ref = sp.eval_ops(sy.ops, x)
        got = E.evaluate_numpy([cols[c] for c in idx], x)
        at = {c: j for j, c in enumerate(idx)}
        np.testing.assert_array_equal(got[:, [at[c] for c in exact]], ref[:, exact])
        for c in install:
            np.testing.assert_allclose(got[:, at[c]], ref[:, c], rtol=1e-14, atol=0)
        seen_nan |= bool(np.isnan(ref[:, exact]).any())
        seen_pos |= bool((ref[:, exact] > 0).any())
    assert seen_pos
