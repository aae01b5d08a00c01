"""The synthetic problems of tests/synth_problem.py, checked without a GPU: the product's
encoder lays the genes out as the oracle does, the inputs make the constraints bite without
saturating, the compact cases fix the intended genes, and every case's shape and expected
kernels are the ones a line of the route table (tests/test_routes_cpu.py) pins."""
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
    want = {"k_slab": 64, "k_last": 1, "k_odd": 57, "k_few": 197, "k_mixed": 40}.get(name, 0)
    assert fixed.sum() == want
    if name == "k_mixed":  # gene 7: fixed in states 0 and 1 only, so it is stored
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
    assert sum(v[6] for v in L) == len(sp.COMPACT) == 5
