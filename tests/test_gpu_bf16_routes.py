"""Every classifier instance of the bf16 perf mode (mv_set_mlp_precision; launch_mlp in
csrc/eval.hip), each at a tolerance measured on the case's own rows instead of a constant:

  k_mlp2<1,BF,DIRECT>    botnet: the shipped net, 756-64-3
  k_mlp2<2,BF,DIRECT>    botnet 756-80-128-3, 756-128-2
  k_mlp2<1,BF,!DIRECT>   LCLD: the shipped net (mlpr_ok is false in bf16), 47-64-8
  k_mlp2<2,BF,!DIRECT>   LCLD 47-96-80-2, 47-128-5
  k_mlpw on LCLD's rows  47-144-272-3, 47-512-2
  k_mlpw<2>, <4>         botnet 756-144-256-2, 756-144-272-2, 756-512-512-256-2, 756-272-144-3
  k_mlp<8,true>          botnet 756-512-512-8 (k_mlpw's LDS passes 160 KiB; its twin 756-512-256-8
                         stays on k_mlpw), m609w (Dm4 624: 19.5 steps of 32 in layer 0)
  k_mlp<4,true>          m1008w (K 144: the half step of dense_mfma_bf)

The CJ / MAXCT instance is pinned by tests/test_routes_cpu.py; the kind is asserted here.

Per case, 3 states x 37 rows through mv_evaluate, min_class (2, 0, 1) from three classes on and
(1, 0, 1) for two: f2 / f3 bit-identical to the fp32 mode's, f1 against tests/bf16_ref.py's
variant A; then a 4-generation attack in bf16 mode whose final f1 is held to variant A on
its final genes.  The tolerance is 4 x floor, floor = the largest pairwise |f1| difference
among the variants A, B and C on the same rows (at least 2^-20), no row left out: the variants
differ in how fp32 accumulation error moves hidden activations across bf16 rounding
boundaries, which is also the device's only legitimate slack (the MFMA's order inside a step of
32 products is not documented).  A floor above 1e-4 fails the case: change its seed.

bias1 is folded in fp32 exactly as k_setup_states folds it (bf16_ref.bias1_fold): an fp64 fold
lies a few fp32 ulps away, enough to put a hidden activation on the other side of a bf16 tie
(botnet-144-256-2, state 2).  Measured floors and errors: DESIGN.md section 4."""
import dataclasses

import numpy as np
import pytest

import bf16_ref
import synth_problem as sp
from oracle import moeva_oracle as mo
from test_gpu_classifier_routes import _classifier, _net, _perturbed_genes, _project
from test_gpu_parity import make_classifier

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 37
FLOOR_MAX = 1e-4
SHIPPED = "shipped"
# m1008w: under the fallback test's row seed (+ 1) one row of state 0 has a hidden activation
# on a bf16 rounding boundary (floor 2.1e-4 > FLOOR_MAX); these rows have none
ROW_SEED = {"m1008w": 2}
CASES = [
    ("botnet", SHIPPED, "k_mlp2(genes)"), ("botnet", (756, 64, 3), "k_mlp2(genes)"),
    ("botnet", (756, 80, 128, 3), "k_mlp2(genes)"), ("botnet", (756, 128, 2), "k_mlp2(genes)"),
    ("lcld", SHIPPED, "k_mlp2"), ("lcld", (47, 64, 8), "k_mlp2"),
    ("lcld", (47, 96, 80, 2), "k_mlp2"), ("lcld", (47, 128, 5), "k_mlp2"),
    ("lcld", (47, 144, 272, 3), "k_mlpw"), ("lcld", (47, 512, 2), "k_mlpw"),
    ("botnet", (756, 144, 256, 2), "k_mlpw"), ("botnet", (756, 144, 272, 2), "k_mlpw"),
    ("botnet", (756, 512, 512, 256, 2), "k_mlpw"), ("botnet", (756, 272, 144, 3), "k_mlpw"),
    ("botnet", (756, 512, 512, 8), "k_mlp"), ("botnet", (756, 512, 256, 8), "k_mlpw"),
    ("m609w", None, "k_mlp"), ("m1008w", None, "k_mlp"),
]


def _id(c):
    return c[0] + ("" if c[1] is None else "-" + (c[1] if c[1] == SHIPPED
                                                  else "-".join(map(str, c[1][1:]))))


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@dataclasses.dataclass
class Setup:
    lay: object
    X: np.ndarray
    ml: tuple
    W: list
    bs: list
    mc: tuple
    genes: np.ndarray
    make_engine: object  # () -> engine with the states bound


def setup(name, dims, tmp_path) -> Setup:
    """The case's problem, net, classes, rows and engine (no GPU call before make_engine())."""
    from moeva2_amd.problem import get_engine

    if dims is None:  # a synthetic fallback case
        sy = sp.build(name, tmp_path)
        mc = sp.min_classes(sy.case)
        genes, _ = sy.eval_genes(np.random.default_rng(sp.case_seed(name) + ROW_SEED.get(name, 1)))

        def make():
            from test_gpu_mlp_fallback import engine_for

            return engine_for(sy)

        return Setup(sy.lay, sy.X, sy.ml, sy.W, sy.bs, mc, genes[:, :N], make)
    p, c, sc = _project(name)
    if dims == SHIPPED:
        clf = make_classifier(name)
        dw = clf.dense_weights()
        W = [np.asarray(w, np.float32) for w in dw.weights]
        bs = [np.asarray(b, np.float32) for b in dw.biases]
    else:
        W, bs = _net(dims, 71)
        clf = _classifier(W, bs)
    mc = (2, 0, 1) if W[-1].shape[1] >= 3 else (1, 0, 1)
    X = p.x[:3]
    probs = [p.problem(X[b], minimize_class=mc[b]) for b in range(3)]
    genes = _perturbed_genes(p, probs, N, np.random.default_rng(72))

    def make():
        eng = get_engine(c, clf, sc, 2)
        bounds = [c.get_feature_min_max(dynamic_input=x) for x in X]
        eng.set_states(X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]),
                       np.array(mc))
        return eng

    return Setup(p.lay, X, p.ml, W, bs, mc, genes, make)


def compare(s: Setup, f1, genes, mut, what):
    """Device f1 (3, n) against variant A under the 4 x floor rule: (floor, error), the worst
    over the states."""
    floor_w = err_w = 0.0
    for b in range(3):
        x_ml = mo.genetic_to_ml(s.lay, genes[b], s.X[b]) * s.ml[0] + s.ml[1]
        ref, floor = bf16_ref.f1_with_floor(x_ml, mut, s.W, s.bs, s.mc[b])
        err = float(np.abs(f1[b] - ref).max())
        print(f"  {what}, state {b}: floor {floor:.3e}, |device - A| {err:.3e}")
        assert floor <= FLOOR_MAX, f"{what}, state {b}: floor {floor:.3e}: change the seed"
        assert err <= 4 * floor, f"{what}, state {b}: {err:.3e} > 4 x floor {floor:.3e}"
        floor_w, err_w = max(floor_w, floor), max(err_w, err)
    return floor_w, err_w


@pytest.mark.parametrize("name,dims,kind", CASES, ids=[_id(c) for c in CASES])
def test_bf16_instance(tmp_path, monkeypatch, name, dims, kind):
    from moeva2_amd._native import NativeError
    from moeva2_amd.attacks.moeva2.ref_dirs import energy_ref_dirs

    monkeypatch.delenv("MV_MLP_V1", raising=False)
    s = setup(name, dims, tmp_path)
    eng = s.make_engine()
    mut = np.asarray(eng.prog.mut_feats)
    gd = torch.as_tensor(s.genes, device="cuda")
    F32 = torch.full((3, N, 3), float("nan"), dtype=torch.float64, device="cuda")
    F16 = torch.full_like(F32, float("nan"))
    try:
        eng.set_mlp_precision("fp32")
        eng.evaluate(gd, F32)
        eng.set_mlp_precision("bf16")
        assert eng.kernel_times()["mlp_kernel"] == kind
        eng.evaluate(gd, F16)
        torch.cuda.synchronize()
        F32, F16 = F32.cpu().numpy(), F16.cpu().numpy()
        np.testing.assert_array_equal(F16[:, :, 1:], F32[:, :, 1:])
        tag = _id((name, dims))
        fl_e, err_e = compare(s, F16[:, :, 0], s.genes, mut, f"{tag} evaluate")
        eng.attack_run(4, 23, 10, 73, energy_ref_dirs(3, 20, 1), 0.05, 0)
        ga = torch.empty((3, 23, s.lay.V), dtype=torch.float64, device="cuda")
        Fa = torch.empty((3, 23, 3), dtype=torch.float64, device="cuda")
        eng.attack_population(ga, Fa)
        torch.cuda.synchronize()
        ga, Fa = ga.cpu().numpy(), Fa.cpu().numpy()
        assert np.isfinite(Fa).all()
        stored = eng.stored_genes()
        if s.lay.ohe_masks:  # one-hot layouts are never compacted
            assert stored.all()
            mut_a = mut
        else:  # the fixed genes' features join the fp32 bias fold
            mut_a = mut[stored]
        fl_a, err_a = compare(s, Fa[:, :, 0], ga, mut_a, f"{tag} attack")
        print(f"bf16 {kind} {tag}: evaluate floor {fl_e:.3e} error {err_e:.3e}; "
              f"attack floor {fl_a:.3e} error {err_a:.3e}")
    except NativeError as e:
        if "error 2" in str(e):  # MV_ERR_HIP: start nothing more on a device that faulted
            pytest.exit(f"{name}: HIP runtime error, session ended: {e}", returncode=3)
        raise
    finally:
        eng.set_mlp_precision("fp32")
