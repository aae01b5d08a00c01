"""k_mlp<MAXCT, BF = false>, the classifier's 32-row-tile fallback (csrc/eval.hip), bit for bit
against oracle/device_order's ``kernel="mlp_v1"`` restatement, on the synthetic problems of
tests/synth_problem.py MLP_CASES (their lines of the route table in tests/test_routes_cpu.py
pin the MAXCT instance, which the kind reported here does not show):

  m609w   512-512-2   k_mlp<8>   the far side of k_mlpw32's LDS guard (m608w: the near side,
                                 checked under ``kernel="mlpw32"``); also with SBX
  m736w   512-272-3   k_mlp<8>   the largest Dm4 this net is accepted at (163,408 B of LDS); 32
                                 and 17 column tiles (wave 0: 8 and 5), 3 classes
  m1008w  144-240-3   k_mlp<4>   the widest problem this net is accepted at; 9 and 15 tiles
  m640n   48-80-2     k_mlp<2>   under MV_MLP_V1: U = 8 with K 48, the ``kk < K`` tail
  m639t   32-16-8     k_mlp<1>   under MV_MLP_V1: waves 2 and 3 without a column tile, 8 classes
(the last two in a child process under the development switches V1_ENV; tests/native/mlp_v1_run.py)

Per case, on 3 states with different x_init and, from 3 classes on, min_class (2, 0, 1):
  a. the classifier kernel the engine reports;
  b. mv_evaluate on 1, 11 and 37 rows per state into NaN-preset outputs (33 rows: the first
     32-row tile spans all three states' bias1 rows, the second holds one live row and 31
     padding rows of state -1): f1 and f2 bit-identical to evaluate_device_order, f3 too (no
     case calls pow), f1 within 1e-5 / 1e-7 of the fp64 forward, f2 / f3 at 1e-12;
  c. a 5-generation attack whose final genes, F and whole "full" history are bit-identical
     to the oracle's engine-order attack (offspring rows through out_map, history writes).
And mv_engine_create refuses 512-272-3 over 752 features and 512-512-2 over 736 (MV_ERR_ARG,
"too large")."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import synth_problem as sp
from oracle import device_order as do
from oracle import moeva_oracle as mo
from test_gpu_row_routes import G_ATT, O_ATT, P_ATT, SEED, _forward64, ref_dirs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = (1, 11, 37)
# (case, MV_MLP_V1, device_order's kernel)
RUNS = [("m608w", False, "mlpw32"), ("m609w", False, "mlp_v1"), ("m736w", False, "mlp_v1"),
        ("m1008w", False, "mlp_v1"), ("m640n", True, "mlp_v1"), ("m639t", True, "mlp_v1")]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth_mlp")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sp.build(name, d)
        return cache[name]

    return get


def engine_for(sy, cx="two_point"):
    from moeva2_amd.attacks.moeva2.classifier import Classifier, DenseMLPModel
    from moeva2_amd.io.tf_bundle import DenseMLP
    from moeva2_amd.problem import get_engine

    if not hasattr(sy, "clf"):
        acts = ["relu"] * (len(sy.W) - 1) + ["softmax"]
        sy.clf = Classifier(DenseMLPModel(DenseMLP(sy.W, sy.bs, acts)))
    eng = get_engine(sy.constraints, sy.clf, sy.scaler, 2)
    eng.set_crossover(cx, 30.0, 0.9)
    xl, xu = sy.bounds()
    eng.set_states(sy.X, xl, xu, np.array(sp.min_classes(sy.case)))
    return eng


def eval_rows(sy):
    genes, _ = sy.eval_genes(np.random.default_rng(sp.case_seed(sy.case.name) + 1))
    return genes[:, :sp.N_PERTURBED]


def device_evaluate(sy, eng):
    """{n: F (B, n, 3)} for n in ROWS, every output preset to NaN."""
    genes, out = eval_rows(sy), {}
    for n in ROWS:
        F = torch.full((sp.B, n, 3), float("nan"), dtype=torch.float64, device="cuda")
        eng.evaluate(torch.as_tensor(np.ascontiguousarray(genes[:, :n]), device="cuda"), F)
        torch.cuda.synchronize()
        out[n] = F.cpu().numpy()
    return out


def device_attack(sy, cx):
    """(genes, F, full history, stored genes) of the 5-generation attack."""
    eng = engine_for(sy, cx)
    try:
        eng.attack_run(G_ATT, P_ATT, O_ATT, SEED, ref_dirs(), 0.05, 2)
        g = torch.empty((sp.B, P_ATT, eng.prog.V), dtype=torch.float64, device="cuda")
        F = torch.empty((sp.B, P_ATT, 3), dtype=torch.float64, device="cuda")
        eng.attack_population(g, F)
        h = torch.empty((sp.B, P_ATT + (G_ATT - 1) * O_ATT, 3 + eng.prog.C), dtype=torch.float64,
                        device="cuda")
        eng.attack_history(h)
        torch.cuda.synchronize()
    finally:
        eng.set_crossover("two_point")
    return g.cpu().numpy(), F.cpu().numpy(), h.cpu().numpy(), eng.stored_genes()


def check_evaluate(sy, Fs, kernel):
    case = sy.case
    genes = eval_rows(sy)
    mc = sp.min_classes(case)
    refs, plains, f64s = [], [], []
    for b, prob in enumerate(sy.probs):
        assert prob.minimize_class == mc[b]
        refs.append(do.evaluate_device_order(prob, genes[b], sy.codes, kernel=kernel))
        plains.append(mo.evaluate(prob, genes[b]))
        x_ml = mo.genetic_to_ml(sy.lay, genes[b], prob.x_init) * sy.ml[0] + sy.ml[1]
        f64s.append(_forward64(x_ml, sy.W, sy.bs)[:, mc[b]])
    worst = 0.0
    for n in ROWS:
        F = Fs[n]
        assert F.shape == (sp.B, n, 3)
        for b in range(sp.B):
            what = f"{case.name} evaluate, {n} rows, state {b}"
            worst = max(worst, float(np.abs(F[b, :, 0] - f64s[b][:n]).max()))
            np.testing.assert_allclose(F[b, :, 0], f64s[b][:n], rtol=1e-5, atol=1e-7, err_msg=what)
            np.testing.assert_allclose(F[b, :, 1], plains[b][:n, 1], rtol=1e-12, atol=1e-15,
                                       err_msg=what)
            np.testing.assert_allclose(F[b, :, 2], plains[b][:n, 2], rtol=1e-12, atol=0,
                                       err_msg=what)
            np.testing.assert_array_equal(F[b], refs[b][:n], err_msg=what)
    return worst


def check_attack(sy, cx, kernel, dev):
    case, lay = sy.case, sy.lay
    g, F, h, stored = dev
    fixed = do.compact_fixed(lay, sy.probs)
    np.testing.assert_array_equal(stored, ~fixed[np.where(lay.mutable_mask)[0]])

    def ev(prob, genes, return_g=False):
        return do.evaluate_device_order(prob, genes, sy.codes, return_g,
                                        fixed=fixed if fixed.any() else None, kernel=kernel)

    worst = 0.0
    mc = sp.min_classes(case)
    for b, prob in enumerate(sy.probs):
        what = f"{case.name} attack {cx}, state {b}"
        r = mo.run_attack(prob, ref_dirs(), G_ATT, P_ATT, O_ATT, SEED, save_history="full",
                          crossover_kind=cx, evaluate_fn=ev, pow_fn=do.det_pow)
        np.testing.assert_array_equal(g[b], r.pop_X, err_msg=what)
        np.testing.assert_array_equal(F[b], r.pop_F, err_msg=what)
        hr = np.concatenate(r.history)
        assert h[b].shape == hr.shape
        np.testing.assert_array_equal(h[b], hr, err_msg=what)
        assert not np.array_equal(g[b], mo.initial_population(prob, P_ATT)), what
        x_ml = mo.genetic_to_ml(lay, g[b], prob.x_init) * sy.ml[0] + sy.ml[1]
        f64 = _forward64(x_ml, sy.W, sy.bs)[:, mc[b]]
        worst = max(worst, float(np.abs(F[b, :, 0] - f64).max()))
        np.testing.assert_allclose(F[b, :, 0], f64, rtol=1e-5, atol=1e-7, err_msg=what)
    return worst


# The narrow nets reach k_mlp only through development switches: MV_MLP_V1 (no k_mlp2; set
# before mv_engine_create, which then has the row kernels write the fp32 ML rows k_mlp reads)
# and, for hidden widths <= 64, MV_MLPR=0 (read once per process: those nets go to k_mlpr
# first).  Hence a child process, as test_plan_overflow_paths_bit_exact runs its build.
V1_ENV = {"m640n": {"MV_MLP_V1": "1"}, "m639t": {"MV_MLP_V1": "1", "MV_MLPR": "0"}}


def run_child(name, out, tmp_path):
    """tests/native/mlp_v1_run.py under the case's switches.  A child that a signal ended (a
    GPU abort or a segmentation fault) or that ran into the time limit ends the session: nothing
    more is started on a device that may have faulted."""
    runner = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "mlp_v1_run.py")
    try:
        r = subprocess.run([sys.executable, runner, out, name, str(tmp_path)],
                           env=dict(os.environ, **V1_ENV[name]), timeout=120)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{name}: the child process hung, session ended", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139, 3):
        pytest.exit(f"{name}: the child process ended with {r.returncode}, session ended",
                    returncode=3)
    assert r.returncode == 0, f"{name}: child exit status {r.returncode}"


def run_device(sy, want_mlp):
    """The device half of a case: (the classifier kernel the engine reports, evaluate outputs,
    attack outputs per crossover)."""
    eng = engine_for(sy)
    kt = eng.kernel_times()
    assert kt["mlp_kernel"] == want_mlp and kt["row_kernel"] == sy.case.row, kt
    Fs = device_evaluate(sy, eng)
    return kt["mlp_kernel"], Fs, {cx: device_attack(sy, cx)
                                  for cx in ["two_point"] + (["sbx"] if sy.case.sbx else [])}


@pytest.mark.parametrize("name,v1,kernel", RUNS, ids=[r[0] for r in RUNS])
def test_mlp_fallback_bit_exact(built, tmp_path, monkeypatch, name, v1, kernel):
    from moeva2_amd._native import NativeError

    sy = built(name)
    case = sy.case
    for k in ("MV_MLP_V1", "MV_MLPR", "MV_XML"):
        monkeypatch.delenv(k, raising=False)
    try:
        if v1:
            # the product route first (kind only), then the switches in a fresh process
            assert engine_for(sy).kernel_times()["mlp_kernel"] == case.mlp
            out = str(tmp_path / "v1.npz")
            run_child(name, out, tmp_path)
            d = np.load(out)
            assert str(d["mlp_kernel"]) == case.mlp_v1 == "k_mlp"  # as the child's engine reported
            Fs = {n: d[f"F{n}"] for n in ROWS}
            att = {"two_point": (d["g"], d["F"], d["h"], d["stored"])}
        else:
            _, Fs, att = run_device(sy, case.mlp)
        worst = check_evaluate(sy, Fs, kernel)
        for cx, dev in att.items():
            worst = max(worst, check_attack(sy, cx, kernel, dev))
    except NativeError as e:
        if "error 2" in str(e):  # MV_ERR_HIP: start nothing more on a device that faulted
            pytest.exit(f"{name}: HIP runtime error, session ended: {e}", returncode=3)
        raise
    print(f"{name} {'-'.join(map(str, case.net))} ({case.note}): "
          f"max |f1 - fp64 forward| {worst:.3e}")


@pytest.mark.parametrize("name,n_plain", [("m736w", 752), ("m609w", 736)])
def test_create_refuses_a_tile_past_the_lds(tmp_path, name, n_plain):
    """The far side of m736w's edge: mlp_lds_bytes of 512-272-3 is 163,408 B at Dm4 736 (the
    case that runs) and 165,456 B > 160 KiB at 752.  And the 512-512-2 net at 736 (164,240 B;
    720: 162,192 B).  The "lds" lines of tests/test_routes_cpu.py."""
    from moeva2_amd._native import NativeError

    case = dataclasses.replace(sp.MLP_BY_NAME[name], n_plain=n_plain)
    sy = sp.Synth(case, tmp_path)
    with pytest.raises(NativeError, match=r"error 1: .*too large"):
        engine_for(sy)
