"""k_survive at its fallback branches, kernel instances and size edges, bit for bit against
mo.survive on the inputs of tests/survival_cases.py (each asserts the witness of the branch it
is built for; tests/test_survival_edges_cpu.py pins the same witnesses on the oracle alone).

Compared per generation and state: n_ranked, order, rank, nadir, niche, dist, survivors and the
carried ideal / worst / extreme / has_extreme.  Output buffers start as NaN / -1, so an entry
the kernel never wrote fails; NaN equals NaN.  wide picks the kernel instance for N <= 512
(mv_survive_wide: 0 = 512 threads, 1 = 576, 2 = 1024) as an attack does from its number of
states; above 512 there is one instance.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import survival_cases as sc  # noqa: E402
from oracle import moeva_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _device_run(case, wide):
    """Every generation of the case through _native.survive; per generation a dict of host
    arrays (outputs and the carried state after the call)."""
    from moeva2_amd import _native

    dev = torch.device("cuda")
    Bn, N, ns = case.F[0].shape[0], case.N, case.n_survive
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    refd = t(case.ref)
    ideal, worst = t(np.full((Bn, 3), np.inf)), t(np.full((Bn, 3), -np.inf))
    ext, has = t(np.zeros((Bn, 9))), t(np.zeros(Bn), torch.int32)
    out = []
    for gen, F in enumerate(case.F):
        i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)
        f64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
        surv, rank, order, nr = i32(Bn, ns), i32(Bn, N), i32(Bn, N), i32(Bn)
        niche, dist, nadir = i32(Bn, N), f64(Bn, N), f64(Bn, 3)
        _native.survive(t(F), refd, ns, sc.MU, case.seed, gen, ideal, worst, ext, has, surv,
                        rank, order, nr, niche, dist, nadir, wide=wide)
        torch.cuda.synchronize()
        h = lambda x: x.cpu().numpy().copy()
        out.append(dict(surv=h(surv), rank=h(rank), order=h(order), nr=h(nr), niche=h(niche),
                        dist=h(dist), nadir=h(nadir), ideal=h(ideal), worst=h(worst),
                        extreme=h(ext), has=h(has)))
    return out


def _compare(case, oracle, got, tag=""):
    eq = np.testing.assert_array_equal
    for gen, (row, g) in enumerate(zip(oracle, got)):
        for b, (r, (ideal, worst, extreme), _w) in enumerate(row):
            ctx = f"{case.name}{tag} gen {gen} state {b}"
            nr = len(np.concatenate(r.fronts))
            assert g["nr"][b] == nr, ctx
            eq(g["order"][b, :nr], np.concatenate(r.fronts), ctx)
            eq(g["rank"][b], np.where(r.rank > 10 ** 15, -1, r.rank), ctx)
            eq(g["nadir"][b], r.nadir, ctx)
            eq(g["niche"][b, :nr], r.niche, ctx)
            eq(g["dist"][b, :nr], r.dist, ctx)
            eq(g["surv"][b], r.survivors, ctx)
            eq(g["ideal"][b], ideal, ctx)
            eq(g["worst"][b], worst, ctx)
            eq(g["extreme"][b].reshape(3, 3), extreme, ctx)
            assert g["has"][b] == 1, ctx


def _check(name, wides=(None,)):
    case, oracle = sc.oracle_run(name)
    sc.check_witness(case, oracle)
    first = None
    for wide in wides:
        got = _device_run(case, wide)
        _compare(case, oracle, got, f" wide {wide}")
        if first is None:
            first = got
        else:  # every instance: the same bits in every buffer, unranked tails included
            for a, b in zip(first, got):
                for k in a:
                    np.testing.assert_array_equal(a[k], b[k], f"{name} wide {wide}: {k}")


@pytest.mark.parametrize("name", sc.BRANCH_CASES)
def test_branches_on_every_instance(name):
    """The five nadir outcomes, the wfront replacement, den0, a small dot, the direction clamp
    on and off, a row at the ideal point, forced ovf (six and exactly five tied directions),
    one +inf and one NaN objective, at N 40 and 303 on the three LDS instances (identical
    results) and at N 600 on the HBM instance."""
    N = sc.oracle_run(name)[0].N
    _check(name, (None, 0, 1, 2) if N <= sc.SURV_NLDS else (None, 2))


def test_wide_outside_0_1_2_is_refused():
    from moeva2_amd import _native

    case, _ = sc.oracle_run("plane-N40")
    for wide in (-1, 3):
        with pytest.raises(_native.NativeError, match="wide must be 0, 1 or 2"):
            _device_run(case, wide)


@pytest.mark.parametrize("name", sc.R_EDGE_CASES)
def test_r_edges(name):
    """R 1..8, both sides of RN 64, SURV_RMAX: even and odd RN with every remainder of the
    sweep's two unrolled loops (the ids state them); wide 1 as well (nine waves)."""
    _check(name, (None, 1))


@pytest.mark.parametrize("name", sc.N_EDGE_CASES)
def test_n_edges(name):
    """N 1, 2, the bitset word edges, the LDS / HBM switch at 512 | 513 and SURV_NMAX, at
    R 20 and R 200; the ids carry surv_offsets' alias (both values on neighbouring N)."""
    _check(name, (None, 2))


def test_n1024_r640():
    """SURV_NMAX with SURV_RMAX: run if mv_survive accepts it, else its LDS refusal."""
    from moeva2_amd import _native

    try:
        _check(sc.N1024_R640)
    except _native.NativeError as e:
        assert "too large for the survival LDS workspace" in str(e)
        _check(sc.n_edge_id(1024, 200))


@pytest.mark.parametrize("name", sc.N_SURVIVE_CASES)
def test_n_survive_edges(name):
    """n_survive 1 and N, exactly on a front boundary (no niching: the witness says so) and
    one past it, and a pure dominance chain of N fronts at N 65 and SURV_NMAX."""
    N = sc.oracle_run(name)[0].N
    _check(name, (None, 1, 2) if N <= sc.SURV_NLDS else (None,))


@pytest.mark.parametrize("name", sc.NICHE_CASES)
def test_niche_sort_switch(name):
    """One front, the fullest niche at NICHE_SORT_MIN and one more: counting | one bitonic sort
    above N 512, counting on both sides at N 512."""
    N = sc.oracle_run(name)[0].N
    _check(name, (None, 2) if N <= sc.SURV_NLDS else (None,))


@pytest.mark.parametrize("P,O", [(2, 1), (2, 2), (3, 7), (64, 32), (65, 32), (1022, 2), (7, 19)])
def test_tournament_selection_edges(P, O):
    """(64, 32): the permutation slots equal P and a power of two; (7, 19): an odd O above P."""
    from moeva2_amd import _native

    Bn = 3
    par = torch.full((Bn, (O + 1) // 2, 2), -1, dtype=torch.int32, device="cuda")
    _native.select_parents(Bn, P, O, 99, 5, par)
    torch.cuda.synchronize()
    ref = mo.tournament_parents(P, O, 99, 5)
    got = par.cpu().numpy()
    for b in range(Bn):
        np.testing.assert_array_equal(got[b], ref)
