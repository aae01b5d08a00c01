"""What k_survive carries from one generation to the next (SurvArgs.carry_flag ...): the
dominance work among survivors that all came from front 0 is skipped, and the survivors'
(niche, dist) are reused while the ideal point and the nadir keep their bits.  Both are
shortcuts for values the kernel would compute again, so every comparison here is exact:
carry on (default) against MV_SURV_CARRY=0 and against the oracle's engine-order attack, and
the device's per-state counters against the counts the oracle's own trajectory gives."""
import os

import numpy as np
import pytest

from conftest import RES
from oracle import moeva_oracle as mo
from oracle.problems import PROJECTS, Project

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class NpScaler:
    def __init__(self, path):
        d = np.load(path)
        self.scale_, self.min_ = d["scale_"], d["min_"]


_REF = {}


def _ref128():
    """energy_ref_dirs(3, 128, seed=1) is not shipped: computed once for the module."""
    from moeva2_amd.attacks.moeva2.ref_dirs import energy_ref_dirs

    if 128 not in _REF:
        _REF[128] = energy_ref_dirs(3, 128, seed=1)
    return _REF[128]


def _constraints(name):
    from moeva2_amd.experiments.united.utils import STR_TO_CONSTRAINTS_CLASS

    feat = os.path.join(RES, PROJECTS[name][0])
    return STR_TO_CONSTRAINTS_CLASS[name](feat, feat.replace("features", "constraints"))


def _engine(name, carry, monkeypatch):
    """A fresh engine; MV_SURV_CARRY is read when the engine is created."""
    from moeva2_amd.attacks.moeva2.classifier import Classifier, load_model
    from moeva2_amd.problem import get_engine

    if carry:
        monkeypatch.delenv("MV_SURV_CARRY", raising=False)
    else:
        monkeypatch.setenv("MV_SURV_CARRY", "0")
    c = _constraints(name)
    clf = Classifier(load_model(os.path.join(RES, PROJECTS[name][1])))
    return get_engine(c, clf, NpScaler(os.path.join(RES, PROJECTS[name][2])), 2), c


def _run(eng, c, X, G, P, O, seed, ref, hist=1):
    """One attack on states X: final genes, F, the reduced history and the two counters."""
    bounds = [c.get_feature_min_max(dynamic_input=x) for x in X]
    eng.set_states(X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]), 1)
    eng.attack_run(G, P, O, seed, ref, 0.05, hist)
    B, V = X.shape[0], eng.prog.V
    g = torch.empty((B, P, V), dtype=torch.float64, device="cuda")
    F = torch.empty((B, P, 3), dtype=torch.float64, device="cuda")
    eng.attack_population(g, F)
    h = np.zeros((B, 0, 3))
    if hist:
        ht = torch.empty((B, P + (G - 1) * O, 3), dtype=torch.float64, device="cuda")
        eng.attack_history(ht)
        h = ht.cpu().numpy()
    torch.cuda.synchronize()
    dom, assoc = eng.survival_carry()
    return g.cpu().numpy(), F.cpu().numpy(), h, dom, assoc


def _oracle(name, c, stored, X, G, P, O, seed, ref, monkeypatch, hist=True):
    """The oracle's engine-order attack of every state, with what each of its survival calls
    would let the next one carry: (results, dom counts, assoc counts).  A call skips
    dominance work when the call before it ranked front 0 only (and the population holds a
    whole 64-row block); it reuses the association when its ideal point and nadir have the
    bits of the call before it."""
    from moeva2_amd.problem import build_device_program
    from oracle import device_order as do

    p = Project(name)
    codes = build_device_program(c).op_code
    fixed = None
    if not stored.all():  # the compact layout (botnet: gene g is mutable feature g)
        fixed = np.zeros(p.lay.mutable_mask.shape[0], bool)
        fixed[np.where(p.lay.mutable_mask)[0][~stored]] = True

    def ev(prob, genes, return_g=False):
        return do.evaluate_device_order(prob, genes, codes, return_g, fixed=fixed)

    calls = []
    survive = mo.survive

    def recording(F, n_survive, st, *a, **k):
        r = survive(F, n_survive, st, *a, **k)
        calls.append((len(r.fronts), st.ideal.copy().view(np.uint64), r.nadir.copy().view(np.uint64)))
        return r

    monkeypatch.setattr(mo, "survive", recording)
    res, dom, assoc = [], [], []
    for x in X:
        calls.clear()
        res.append(mo.run_attack(p.problem(x), ref, G, P, O, seed,
                                 save_history="reduced" if hist else None, evaluate_fn=ev,
                                 pow_fn=do.det_pow))
        assert len(calls) == G
        dom.append(sum(calls[g - 1][0] == 1 for g in range(1, G)) if P >= 64 else 0)
        assoc.append(sum(np.array_equal(calls[g][1], calls[g - 1][1]) and
                         np.array_equal(calls[g][2], calls[g - 1][2]) for g in range(1, G)))
    monkeypatch.setattr(mo, "survive", survive)
    return res, np.array(dom), np.array(assoc)


def _compare(name, X, G, P, O, seed, ref, monkeypatch, hist=1):
    """Carry on == carry off == oracle (genes, F, history), counters == the oracle's counts
    (zero with the knob off).  Returns the counters."""
    on, c = _engine(name, True, monkeypatch)
    g1, F1, h1, dom, assoc = _run(on, c, X, G, P, O, seed, ref, hist)
    stored = on.stored_genes()
    off, c0 = _engine(name, False, monkeypatch)
    g0, F0, h0, dom0, assoc0 = _run(off, c0, X, G, P, O, seed, ref, hist)
    assert not dom0.any() and not assoc0.any()
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(F1, F0)
    np.testing.assert_array_equal(h1, h0)
    res, odom, oassoc = _oracle(name, c, stored, X, G, P, O, seed, ref, monkeypatch, bool(hist))
    for b, r in enumerate(res):
        np.testing.assert_array_equal(g1[b], r.pop_X)
        np.testing.assert_array_equal(F1[b], r.pop_F)
        if hist:
            np.testing.assert_array_equal(h1[b], np.concatenate(r.history))
    print(f"{name} P={P} O={O} G={G}: dominance shortcut device {dom} oracle {odom}; "
          f"association reuse device {assoc} oracle {oassoc}")
    np.testing.assert_array_equal(dom, odom)
    np.testing.assert_array_equal(assoc, oassoc)
    return dom, assoc


def test_mixed_paths_attack(monkeypatch):
    """Botnet states on which both shortcuts and both fallbacks run within 40 generations
    (P = 131, N = 191: two whole survivor blocks and a mixed one): bit-identical results, and
    the device took each path in exactly the generations the oracle's trajectory says."""
    X = Project("botnet").x[[50, 100, 150, 250, 300, 386]]
    G = 40
    dom, assoc = _compare("botnet", X, G, 131, 60, 42, _ref128(), monkeypatch)
    # not vacuous: shortcut and fallback both ran, for both mechanisms, on at least 3 states
    assert ((dom > 0) & (dom < G - 1)).sum() >= 3, dom
    assert ((assoc > 0) & (assoc < G - 1)).sum() >= 3, assoc


@pytest.mark.parametrize("n_pop", [61, 60])
def test_whole_block_edges(n_pop, monkeypatch):
    """P = 64: exactly one whole survivor block (one block pair skipped); P = 63: none."""
    from moeva2_amd.attacks.moeva2.ref_dirs import riesz_energy_dirs

    X = Project("botnet").x[[50, 100, 150]]
    P = n_pop + 3
    dom, _ = _compare("botnet", X, 15, P, 20, 42,
                      riesz_energy_dirs(3, n_pop, seed=1, n_max_iter=200), monkeypatch)
    if P < 64:
        assert not dom.any()
    else:
        assert dom.any()


def test_hbm_bitsets(monkeypatch):
    """N = 545 > 512: the dominance bitsets live in HBM and whole block pairs are skipped
    (P = 515: eight whole survivor blocks).  LCLD, as the full-size test of this path; its f3
    is pinned to the oracle within 1 ulp there, so here the oracle gives the counters and
    carry on / off must agree bit for bit."""
    from moeva2_amd.attacks.moeva2.ref_dirs import energy_ref_dirs

    name, G, P, O, seed = "lcld", 4, 515, 30, 42
    X = Project(name).x[:2]
    ref = energy_ref_dirs(3, 200, seed=1)
    on, c = _engine(name, True, monkeypatch)
    g1, F1, h1, dom, assoc = _run(on, c, X, G, P, O, seed, ref)
    off, c0 = _engine(name, False, monkeypatch)
    g0, F0, h0, dom0, assoc0 = _run(off, c0, X, G, P, O, seed, ref)
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(F1, F0)
    np.testing.assert_array_equal(h1, h0)
    assert not dom0.any() and not assoc0.any()
    res, odom, oassoc = _oracle(name, c, on.stored_genes(), X, G, P, O, seed, ref, monkeypatch)
    for b, r in enumerate(res):
        np.testing.assert_array_equal(g1[b], r.pop_X)  # the oracle ran this trajectory
    print(f"lcld N={P + O}: dominance shortcut device {dom} oracle {odom}; association reuse "
          f"device {assoc} oracle {oassoc}")
    np.testing.assert_array_equal(dom, odom)
    np.testing.assert_array_equal(assoc, oassoc)
    assert dom.all(), dom  # the block-pair shortcut ran on both states


def test_reset_between_attacks(monkeypatch):
    """Two attacks on one engine, the second on other states: nothing of the first attack is
    carried into the second (its results and counters are those of a fresh engine)."""
    p = Project("botnet")
    ref = _ref128()
    G, P, O = 12, 131, 60
    eng, c = _engine("botnet", True, monkeypatch)
    first = _run(eng, c, p.x[[50, 100, 150, 250]], G, P, O, 42, ref)
    assert first[3].any() and first[4].any()
    second = _run(eng, c, p.x[[300, 386, 100]], G, P, O, 42, ref)
    again = _run(eng, c, p.x[[300, 386, 100]], G, P, O, 42, ref)  # same binding size, no realloc
    fresh_eng, c1 = _engine("botnet", True, monkeypatch)
    fresh = _run(fresh_eng, c1, p.x[[300, 386, 100]], G, P, O, 42, ref)
    for got in (second, again):
        for a, b in zip(got, fresh):
            np.testing.assert_array_equal(a, b)


def test_dense_survival_carries_nothing(monkeypatch):
    """mv_survive on a stand-alone merged F has no previous generation: calls on the same F,
    the second of each pair after a call whose survivors would qualify for both shortcuts,
    return the oracle's survivors, and the counters of the process's engine stay zero."""
    from moeva2_amd import _native as nat

    p = Project("botnet")
    ref_h = _ref128()
    eng, c = _engine("botnet", True, monkeypatch)
    X = p.x[[50, 100]]
    bounds = [c.get_feature_min_max(dynamic_input=x) for x in X]
    eng.set_states(X, np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds]), 1)
    rng = np.random.default_rng(3)
    B, N, n_survive = 2, 191, 131
    Fh = rng.random((B, N, 3))
    Fh[:, :n_survive, 0] = 1.0 - Fh[:, :n_survive, 1]  # a mutually non-dominated head
    F = torch.from_numpy(Fh).cuda()
    ref = torch.from_numpy(ref_h).cuda()
    out = []
    for _ in range(2):  # the second call sees the first one's ideal / worst / extremes
        st = dict(ideal=torch.full((B, 3), float("inf"), dtype=torch.float64, device="cuda"),
                  worst=torch.full((B, 3), float("-inf"), dtype=torch.float64, device="cuda"),
                  extreme=torch.zeros((B, 9), dtype=torch.float64, device="cuda"),
                  has=torch.zeros(B, dtype=torch.int32, device="cuda"))
        surv = torch.empty((B, n_survive), dtype=torch.int32, device="cuda")
        for gen in (1, 1):
            nat.survive(F, ref, n_survive, 0.05, 7, gen, st["ideal"], st["worst"], st["extreme"],
                        st["has"], surv)
            torch.cuda.synchronize()
            out.append(surv.cpu().numpy().copy())
    np.testing.assert_array_equal(out[0], out[2])
    np.testing.assert_array_equal(out[1], out[3])
    asp = np.full((1, 3), 1.0 / 3.0)
    for b in range(B):
        ost = mo.SurvivalState()
        for k in range(2):
            r = mo.survive(Fh[b], n_survive, ost, ref_h, asp, 0.05, 7, 1)
            np.testing.assert_array_equal(out[k][b], r.survivors)
    dom, assoc = eng.survival_carry()
    assert not dom.any() and not assoc.any()
