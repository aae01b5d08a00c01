"""Every instance family of the row kernels (k_narrow, k_gen + k_cons, k_genc: csrc/routes.h
row_route / vary_nt / genc_nt), each pinned on a synthetic problem at the shape where its guards
change side (tests/synth_problem.py: the case table with what each shape reaches; its line of
the route table in tests/test_routes_cpu.py pins the NT / NV / FULL / SLIM instance, which the
kind reported here does not show).  The shipped problems give these kernels four shapes only.

Per case, on 3 states:
  a. the row and the classifier kernel kinds the engine reports;
  b. mv_evaluate on 37 perturbed rows per state plus rows with a zero RATIO_SAFE denominator
     and, for FULL programs, a RATIO_MASKED denominator of 0, of 5e-324 (the quotient is inf)
     and of inf: F against the plain oracle (f1 rtol 1e-5 atol 1e-7, f2 / f3 rtol 1e-12) and
     bit for bit against the oracle in the engine's order.  On the row with the infinite gene
     f1 is not compared (the classifier's fp32 input is inf there, and numpy's relu keeps a
     NaN that the hardware's max drops: not the row kernels' business); f2 and f3 are;
  c. mv_variation (P 40, O 24: the k_gen instance of the shape) against the oracle's crossover
     + mutation: bit-identical with the engine's pow, integer genes exact and real genes
     1e-12 with np.power;
  d. a 5-generation attack (P 23, O 10, full history): final genes, F and every history
     column bit-identical to the oracle's engine-order attack (f3 / G at 1e-14 for the one
     case with an LCLD_INSTALL column, whose pow is the device library's);
  e. narrow cases: the same attack under MV_NARROW=0 is bit-identical;
  f. cases with MV_OP_EXPR columns (the x cases: k_gen + k_consx<IDENT, NT>, all ten instances,
     with all or a third of the columns restated as expressions): the twin -- the same problem
     with every column a dedicated op, on whichever kernels its shape takes, k_genc from 129
     genes on -- runs the same attack: populations, f1, f2 and every G column of the history
     bit-identical, f3 within (C - 1) 2^-53 relative (equal non-negative terms summed in
     another lane order; DESIGN.md section 7b's guarantee, checked across routes).
Cases marked so run a second time with crossover="sbx"; c129 and c384 also run under the
plan-overflow build (tests/native/planovf_synth_run.py) with bit-identical populations."""
import os
import subprocess
import sys

import numpy as np
import pytest

import synth_problem as sp
from oracle import device_order as do
from oracle import moeva_oracle as mo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# seed 7: every case's population changes in every state within these 5 generations (found on
# the oracle alone; every state draws the same mutations, and k_few's 3 stored genes of 200 are
# hit by few of them; a case whose own ``seed`` is set states its reason in synth_problem.py)
G_ATT, P_ATT, O_ATT, SEED = 5, 23, 10, 7
RUNS = [(c.name, "two_point") for c in sp.CASES] + [(c.name, "sbx") for c in sp.CASES if c.sbx]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth")
    cache = {}

    def get(name, twin=False):
        if (name, twin) not in cache:
            case = sp.CASES_BY_NAME[name]
            cache[name, twin] = sp.build(sp.twin(case) if twin else case, d)
        return cache[name, twin]

    return get


_REF = []


def ref_dirs():
    from moeva2_amd.attacks.moeva2.ref_dirs import energy_ref_dirs

    if not _REF:
        _REF.append(energy_ref_dirs(3, P_ATT - 3, 1))
    return _REF[0]


def engine_for(sy, cx):
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.io.tf_bundle import DenseMLP
    from moeva2_amd.problem import get_engine

    if not hasattr(sy, "clf"):
        sy.clf = Classifier(DenseMLPModel(DenseMLP(sy.W, sy.bs, ["relu", "relu", "softmax"])))
    eng = get_engine(sy.constraints, sy.clf, sy.scaler, 2)
    eng.set_crossover(cx, 30.0, 0.9)
    xl, xu = sy.bounds()
    eng.set_states(sy.X, xl, xu, 1)
    return eng


def run_attack(sy, cx, hist=2):
    """The device attack of item d: (engine, genes, F, history) as numpy arrays."""
    eng = engine_for(sy, cx)
    try:
        eng.attack_run(G_ATT, P_ATT, O_ATT, sy.case.seed or SEED, ref_dirs(), 0.05, hist)
        V, C = eng.prog.V, eng.prog.C
        g = torch.empty((sp.B, P_ATT, V), dtype=torch.float64, device="cuda")
        F = torch.empty((sp.B, P_ATT, 3), dtype=torch.float64, device="cuda")
        eng.attack_population(g, F)
        h = None
        if hist:
            h = torch.empty((sp.B, P_ATT + (G_ATT - 1) * O_ATT, 3 + C), dtype=torch.float64,
                            device="cuda")
            eng.attack_history(h)
        torch.cuda.synchronize()
    finally:
        eng.set_crossover("two_point")
    return eng, g.cpu().numpy(), F.cpu().numpy(), None if h is None else h.cpu().numpy()


def _forward64(x_ml, W, bs):
    """The fp32 weights and the fp32-cast input, every operation in fp64."""
    h = np.asarray(x_ml, np.float64).astype(np.float32).astype(np.float64)
    for i, (w, b) in enumerate(zip(W, bs)):
        h = h @ w.astype(np.float64) + b.astype(np.float64)
        if i + 1 < len(W):
            h = np.maximum(h, 0.0)
    e = np.exp(h - h.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _f3_equal(case, got, ref, what):
    if case.install:  # device pow against numpy's: an ulp in a violated column
        np.testing.assert_allclose(got, ref, rtol=1e-14, atol=0, err_msg=what)
    else:
        np.testing.assert_array_equal(got, ref, err_msg=what)


def check_evaluate(sy, eng):
    case = sy.case
    genes, inf_rows = sy.eval_genes(np.random.default_rng(sp.case_seed(case.name) + 1))
    n = genes.shape[1]
    F = torch.empty((sp.B, n, 3), dtype=torch.float64, device="cuda")
    eng.evaluate(torch.as_tensor(genes, device="cuda"), F)
    torch.cuda.synchronize()
    F = F.cpu().numpy()
    fin = np.setdiff1d(np.arange(n), inf_rows)
    worst = 0.0
    for b, prob in enumerate(sy.probs):
        what = f"{case.name} evaluate, state {b}"
        plain = mo.evaluate(prob, genes[b])
        x_ml = mo.genetic_to_ml(sy.lay, genes[b][fin], prob.x_init) * sy.ml[0] + sy.ml[1]
        worst = max(worst, float(np.abs(F[b, fin, 0] - _forward64(x_ml, sy.W, sy.bs)[:, 1]).max()))
        np.testing.assert_allclose(F[b, fin, 0], plain[fin, 0], rtol=1e-5, atol=1e-7, err_msg=what)
        np.testing.assert_allclose(F[b, :, 1], plain[:, 1], rtol=1e-12, atol=1e-15, err_msg=what)
        np.testing.assert_allclose(F[b, :, 2], plain[:, 2], rtol=1e-12, atol=0, err_msg=what)
        ref = do.evaluate_device_order(prob, genes[b], sy.codes)
        np.testing.assert_array_equal(F[b, fin, 0], ref[fin, 0], err_msg=what)
        np.testing.assert_array_equal(F[b, :, 1], ref[:, 1], err_msg=what)
        _f3_equal(case, F[b, :, 2], ref[:, 2], what)
    return worst


def check_variation(sy, eng, cx):
    lay = sy.lay
    P, O = 40, 24
    types = mo.genetic_types(lay)
    masks = [np.array([t == "real" for t in types]), np.array([t == "int" for t in types])]
    isr = masks[0]
    rng = np.random.default_rng(3)
    pops, gls, gus = [], [], []
    for prob in sy.probs:
        gl, gu = mo.genetic_bounds(lay, prob.xl, prob.xu)
        g = rng.uniform(gl, gu, size=(P, lay.V))
        g[:, ~isr] = np.round(g[:, ~isr])
        g[:5] = mo.initial_population(prob, 1)[0]
        pops.append(g)
        gls.append(gl)
        gus.append(gu)
    parents = mo.tournament_parents(P, O, 99, 5)
    par = torch.as_tensor(np.tile(parents[None], (sp.B, 1, 1)).astype(np.int32), device="cuda")
    off = torch.empty((sp.B, O, lay.V), dtype=torch.float64, device="cuda")
    eng.variation(P, O, 99, 5, torch.as_tensor(np.stack(pops), device="cuda"), par, off)
    torch.cuda.synchronize()
    got = off.cpu().numpy()
    for b in range(sp.B):
        what = f"{sy.case.name} variation {cx}, state {b}"
        pX = np.stack([pops[b][parents[:, 0]], pops[b][parents[:, 1]]])

        def children(pow_fn):
            if cx == "sbx":
                c = mo.sbx_crossover(pX, masks, gls[b], gus[b], 99, 5, 30.0, 0.9,
                                     pow_fn=pow_fn)[:O]
            else:
                c = mo.crossover(pX, masks, 99, 5)[:O]
            return mo.mutation(c, gls[b], gus[b], types, 99, 5, pow_fn=pow_fn)

        ref_np = children(np.power)
        np.testing.assert_array_equal(got[b][:, ~isr], ref_np[:, ~isr], err_msg=what)
        np.testing.assert_allclose(got[b][:, isr], ref_np[:, isr], rtol=1e-12, atol=1e-12,
                                   err_msg=what)
        np.testing.assert_array_equal(got[b], children(do.det_pow), err_msg=what)


def check_attack(sy, cx):
    case, lay = sy.case, sy.lay
    eng, g, F, h = run_attack(sy, cx)
    stored = eng.stored_genes()
    fixed = do.compact_fixed(lay, sy.probs)
    mut = np.where(lay.mutable_mask)[0]
    if case.ident:
        np.testing.assert_array_equal(stored, ~fixed[mut])
    else:
        assert stored.all() and not fixed.any()
    assert (~stored).sum() == sp.N_FIXED.get(case.name, 0)

    def ev(prob, genes, return_g=False):
        return do.evaluate_device_order(prob, genes, sy.codes, return_g,
                                        fixed=fixed if fixed.any() else None)

    isi = mo.genetic_types(lay) != "real"
    worst = 0.0
    for b, prob in enumerate(sy.probs):
        what = f"{case.name} attack {cx}, state {b}"
        r = mo.run_attack(prob, ref_dirs(), G_ATT, P_ATT, O_ATT, case.seed or SEED,
                          save_history="full",
                          crossover_kind=cx, evaluate_fn=ev, pow_fn=do.det_pow)
        np.testing.assert_array_equal(g[b], r.pop_X, err_msg=what)
        np.testing.assert_array_equal(F[b, :, :2], r.pop_F[:, :2], err_msg=what)
        _f3_equal(case, F[b, :, 2], r.pop_F[:, 2], what)
        hr = np.concatenate(r.history)
        assert h[b].shape == hr.shape
        np.testing.assert_array_equal(h[b][:, :2], hr[:, :2], err_msg=what)
        _f3_equal(case, h[b][:, 2:], hr[:, 2:], what)
        assert not np.array_equal(g[b], mo.initial_population(prob, P_ATT)), what
        gl, gu = mo.genetic_bounds(lay, prob.xl, prob.xu)
        assert (np.rint(g[b][:, isi]) == g[b][:, isi]).all(), what
        assert (g[b] >= gl).all() and (g[b] <= gu).all(), what
        x_ml = mo.genetic_to_ml(lay, g[b], prob.x_init) * sy.ml[0] + sy.ml[1]
        worst = max(worst, float(np.abs(F[b, :, 0] - _forward64(x_ml, sy.W, sy.bs)[:, 1]).max()))
        np.testing.assert_allclose(F[b, :, 0], mo.evaluate(prob, g[b])[:, 0], rtol=1e-5, atol=1e-7)
    return (g, F, h), worst


def check_twin(sy, tw, dev):
    """Item f: ``dev`` = (genes, F, history) of the attack with EXPR columns."""
    g, F, h = dev
    eng, g2, F2, h2 = run_attack(tw, "two_point")
    what = f"{sy.case.name} against its all-dedicated twin"
    assert eng.prog.C == sy.case.C and (np.asarray(tw.codes) != 16).all()
    np.testing.assert_array_equal(g, g2, err_msg=what)
    np.testing.assert_array_equal(F[..., :2], F2[..., :2], err_msg=what)
    np.testing.assert_array_equal(h[..., :2], h2[..., :2], err_msg=what)
    np.testing.assert_array_equal(h[..., 3:], h2[..., 3:], err_msg=what)
    rtol = (sy.case.C - 1) * 2.0 ** -53
    np.testing.assert_allclose(F[..., 2], F2[..., 2], rtol=rtol, atol=0, err_msg=what)
    np.testing.assert_allclose(h[..., 2], h2[..., 2], rtol=rtol, atol=0, err_msg=what)
    return eng.kernel_times()["row_kernel"]


@pytest.mark.parametrize("name,cx", RUNS, ids=[f"{n}-{c}" for n, c in RUNS])
def test_row_route(built, monkeypatch, name, cx):
    from moeva2_amd._native import NativeError

    try:
        _row_route(built(name), monkeypatch, name, cx, built)
    except NativeError as e:
        if "error 2" in str(e):  # MV_ERR_HIP: start nothing more on a device that faulted
            pytest.exit(f"{name} {cx}: HIP runtime error, session ended: {e}", returncode=3)
        raise


def _row_route(sy, monkeypatch, name, cx, built):
    case = sy.case
    monkeypatch.delenv("MV_NARROW", raising=False)
    eng = engine_for(sy, cx)
    try:
        kt = eng.kernel_times()
        assert kt["row_kernel"] == ((case.row_sbx or case.row) if cx == "sbx" else case.row)
        assert kt["mlp_kernel"] == case.mlp
        worst = check_evaluate(sy, eng) if cx == "two_point" else 0.0
        check_variation(sy, eng, cx)
    finally:
        eng.set_crossover("two_point")
    dev, w2 = check_attack(sy, cx)
    if name in sp.NARROW and cx == "two_point":  # e. the wave-per-row kernels on the same rows
        monkeypatch.setenv("MV_NARROW", "0")
        _, g0, F0, h0 = run_attack(sy, cx)
        np.testing.assert_array_equal(dev[0], g0)
        np.testing.assert_array_equal(dev[1], F0)
        np.testing.assert_array_equal(dev[2], h0)
    twin = ""
    if case.expr and cx == "two_point":  # f. the same program as dedicated ops
        twin = ", twin on " + check_twin(sy, built(name, twin=True), dev)
    print(f"{name} {cx} ({case.note}{twin}): max |f1 - fp64 forward| {max(worst, w2):.3e}")


PLANOVF_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir,
                           "moeva2-ijcai22-replication_amd", "lib",
                           "libmoeva_mi355x_planovf.so")
_OVF = [(c.name, cx) for c in sp.CASES if c.planovf for cx in ("two_point", "sbx")]


@pytest.mark.parametrize("name,cx", _OVF, ids=[f"{n}-{c}" for n, c in _OVF])
def test_plan_overflow_build_bit_exact(built, tmp_path, name, cx):
    """k_genc's plan-overflow paths (the `make planovf` build flags every row with two or more
    stored mutations) at NT 4 and NT 6, in a fresh process as test_plan_overflow_paths_bit_exact
    runs botnet: the populations equal the default build's."""
    if not os.path.exists(PLANOVF_LIB):
        pytest.fail(f"{PLANOVF_LIB} missing: build it with `make -C "
                    "moeva2-ijcai22-replication_amd/csrc planovf` (__graft_entry__.build())")
    out = str(tmp_path / "planovf.npz")
    runner = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native",
                          "planovf_synth_run.py")
    subprocess.run([sys.executable, runner, out, name, cx, str(tmp_path)],
                   env=dict(os.environ, MOEVA_MI355X_LIB=PLANOVF_LIB), check=True, timeout=240)
    d = np.load(out)
    _, g, F, _ = run_attack(built(name), cx, hist=0)
    np.testing.assert_array_equal(d["genes"], g)
    np.testing.assert_array_equal(d["F"], F)
