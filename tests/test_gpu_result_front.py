"""The result kernels (csrc/survive.hip: k_front_mask, k_front_scan, k_front_gather,
k_gather_pop) at their shape edges.  The suite ran them at P 43 and B 7 only: one 64-lane
ballot chunk, one pass of the 256-thread loops, one state per scan thread, and asserted nothing
about dominated members.

Through mv_attack_front / mv_attack_population on attacks of an 8-gene synthetic problem
(tests/synth_problem.py "n8p"): ``front`` equals moeva2._non_dominated on the final F,
``offsets`` is the exclusive cumsum of the front sizes, the first offsets[B] rows of X / Fx are
genes[b][nd] / F[b][nd] in population order, bit for bit; every output starts as a sentinel
(with a guard row), so an element a kernel does not write, or writes past the end, cannot pass.
P 63 | 64 | 65, 255 | 256 | 257 and 1022 (the largest pop_size mv_attack_run accepts); X only,
Fx only, neither, the engine's own mask / offsets scratch; a compact layout ("k_last"); B 1025
and 2500.  A final population rarely holds a dominated member (see SIZES): the cases at P 63
and 65, the argument variants and the many-state cases at G 30 run attacks, found on the oracle,
that end with one, and assert it.

Through mv_front (the same three kernels on a caller's F) on populations built for the
relation: ties, duplicates, chains, infinities, NaN, -0.0, fronts of 1 .. P members scattered
over the population, at every P above and at B 1025 / 2500 with front sizes 1..5.
"""
import numpy as np
import pytest

import synth_problem as sp
from oracle import moeva_oracle as mo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 7


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth_front")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sp.build(name, d)
        return cache[name]

    return get


def attack(sy, P, O, G, B=sp.B, first=None):
    """A G-generation attack on B states (the case's three, repeated): the engine, ready for
    mv_attack_population / mv_attack_front.  ``first``: state b draws from its own random
    stream first + b (the oracle's run_attack(stream_key=first + b)); None: shared draws."""
    from test_gpu_row_routes import engine_for, ref_dirs

    eng = engine_for(sy, "two_point")
    if B != sp.B or first is not None:
        idx = np.arange(B) % sp.B
        xl, xu = sy.bounds()
        eng.set_state_streams(first is not None, first or 0)
        eng.set_states(sy.X[idx], xl[idx], xu[idx], 1)
    try:
        eng.attack_run(G, P, O, SEED, ref_dirs(), 0.05, 0)
    finally:
        eng.set_state_streams(False, 0)
    return eng


def population(eng, B, P):
    V = eng.prog.V
    g = torch.full((B, P, V), float("nan"), dtype=torch.float64, device="cuda")
    F = torch.full((B, P, 3), float("nan"), dtype=torch.float64, device="cuda")
    eng.attack_population(g, F)
    torch.cuda.synchronize()
    return g.cpu().numpy(), F.cpu().numpy()


def front(eng, B, P, mask=True, offsets=True, X=True, Fx=True):
    """mv_attack_front into sentinel-filled tensors: (front, offsets, X, Fx) as numpy arrays,
    None for the ones not passed.  X and Fx carry one guard row after the B * P the engine may
    fill: it must stay a sentinel like every row past offsets[B]."""
    V = eng.prog.V
    n = B * P + 1
    t = [torch.full((B, P), 7, dtype=torch.uint8, device="cuda") if mask else None,
         torch.full((B + 1,), -1, dtype=torch.int32, device="cuda") if offsets else None,
         torch.full((n, V), float("nan"), dtype=torch.float64, device="cuda") if X else None,
         torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda") if Fx else None]
    eng.attack_front(*t)
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in t]


def expected(genes, F):
    from moeva2_amd.attacks.moeva2.moeva2 import _non_dominated

    nd = np.stack([_non_dominated(F[b]) for b in range(F.shape[0])])
    off = np.concatenate([[0], np.cumsum(nd.sum(axis=1))]).astype(np.int32)
    return nd, off, np.concatenate([genes[b][nd[b]] for b in range(F.shape[0])]), \
        np.concatenate([F[b][nd[b]] for b in range(F.shape[0])])


def check_front(got, want, what, states=None):
    fr, off, X, Fx = got
    nd, woff, wX, wFx = want
    if fr is not None:
        np.testing.assert_array_equal(fr, nd.astype(np.uint8), err_msg=f"{what}: front")
    if off is not None:
        assert off[0] == 0, what
        np.testing.assert_array_equal(off, woff, err_msg=f"{what}: offsets")
    n = int(woff[-1])
    rows = (np.arange(n) if states is None else
            np.concatenate([np.arange(woff[b], woff[b + 1]) for b in states]))
    if X is not None:
        np.testing.assert_array_equal(X[rows], wX[rows], err_msg=f"{what}: X")
        assert np.isnan(X[n:]).all(), f"{what}: rows past offsets[B] were written"
    if Fx is not None:
        np.testing.assert_array_equal(Fx[rows], wFx[rows], err_msg=f"{what}: Fx")
        assert np.isnan(Fx[n:]).all(), f"{what}: rows past offsets[B] were written"


def report(what, nd, genes):
    """(states with a dominated member, states with more than one distinct member)."""
    B = nd.shape[0]
    moved = sum(int((genes[b] != genes[b][:1]).any()) for b in range(B))
    partial = int((~nd.all(axis=1)).sum())
    print(f"{what}: {partial} of {B} states with a dominated member, {moved} with more than "
          "one distinct member")
    return partial, moved


# ------------------------------------------------------------------ fronts of attacks
# the largest pop_size: P + O <= 1024 with an even O >= 2
P_MAX = 1022
# (P, O, G, key).  Survival fills the population front by front and the copies of the initial
# state (f2 = 0) cannot be dominated, so a final population holds a dominated member only when
# the merged first front of the last generation is smaller than P: about one attack in a
# hundred of these.  ``key`` names a random stream, found on the oracle alone (whose attacks
# equal the engine's bit for bit: tests/test_gpu_row_routes.py), whose attack on state key % 3
# ends that way; the case runs per-state streams key - key % 3 .. and asserts the dominated
# member.  No such stream was found for the sizes with key None (P 1022 with its 2 offspring
# per generation keeps ~1000 copies of the initial state for hundreds of generations): their
# fronts are full, and the dominated rows of those sizes are test_front_kernels_on_any_F's.
SIZES = [(63, 20, 60, 215), (64, 20, 4, None), (65, 20, 60, 20), (255, 40, 4, None),
         (256, 40, 4, None), (257, 40, 4, None), (P_MAX, 2, 4, None)]


@pytest.mark.parametrize("P,O,G,key", SIZES, ids=[f"P{s[0]}" for s in SIZES])
def test_front_population_sizes(built, P, O, G, key):
    sy = built("n8p")
    eng = attack(sy, P, O, G, first=None if key is None else key - key % 3)
    genes, F = population(eng, sp.B, P)
    assert np.isfinite(genes).all() and np.isfinite(F).all()
    want = expected(genes, F)
    check_front(front(eng, sp.B, P), want, f"P {P}")
    partial, moved = report(f"P {P} O {O} G {G} stream {key}", want[0], genes)
    assert moved == sp.B  # the populations moved
    if key is not None:
        assert not want[0][key % 3].all(), f"P {P}: state {key % 3} has no dominated member"


def test_front_upper_limit_is_the_engines(built):
    """mv_attack_run refuses P + O > 1024, so P 1022 is the largest population a front is ever
    taken of (k_front_mask's and k_front_gather's LDS arrays hold that many members); mv_front
    refuses more as well."""
    from moeva2_amd import _native
    from test_gpu_row_routes import engine_for, ref_dirs

    eng = engine_for(built("n8p"), "two_point")
    with pytest.raises(_native.NativeError, match="bad attack parameters"):
        eng.attack_run(2, P_MAX + 1, 2, SEED, ref_dirs(), 0.05, 0)
    F = torch.zeros((1, P_MAX + 1, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(_native.NativeError, match="bad mv_front arguments"):
        _native.front(F, torch.zeros((1, P_MAX + 1), dtype=torch.uint8, device="cuda"),
                      torch.zeros(2, dtype=torch.int32, device="cuda"))


def test_front_first_generation_is_all_front(built):
    """G = 1: P copies of the initial state, none dominates another."""
    P = 65
    eng = attack(built("n8p"), P, 20, 1)
    genes, F = population(eng, sp.B, P)
    want = expected(genes, F)
    assert want[0].all() and (genes == genes[:, :1]).all()
    check_front(front(eng, sp.B, P), want, "G 1")


@pytest.mark.parametrize("variant", ["X", "Fx", "neither", "scratch"])
def test_front_argument_variants(built, variant):
    """On the P 65 attack whose state 2 ends with dominated members."""
    P, O, G, key = SIZES[2]
    eng = attack(built("n8p"), P, O, G, first=key - key % 3)
    want = expected(*population(eng, sp.B, P))
    assert not want[0][key % 3].all()
    if variant == "scratch":  # the engine's own mask / offsets, allocated by the first call
        for call in range(2):
            got = front(eng, sp.B, P, mask=False, offsets=False)
            check_front(got, want, f"scratch, call {call}")
        got = front(eng, sp.B, P, mask=False)  # one of the two from the caller
        check_front(got, want, "scratch mask, caller's offsets")
        assert got[1] is not None
    else:
        got = front(eng, sp.B, P, X=variant == "X", Fx=variant == "Fx")
        assert (got[2] is None) == (variant != "X") and (got[3] is None) == (variant != "Fx")
        check_front(got, want, variant)


def test_front_compact_layout(built, monkeypatch):
    """"k_last": 200 genes, the last one fixed in every state (199 stored).  k_front_gather and
    k_gather_pop expand the stored genes through cmap and fill the fixed one from the state's
    bound; the run equals the full layout's.  (Fronts full: see SIZES.)"""
    P, O, G = 65, 20, 4
    sy = built("k_last")
    monkeypatch.delenv("MV_COMPACT", raising=False)
    eng = attack(sy, P, O, G)
    stored = eng.stored_genes()
    assert (~stored).sum() == 1 and not stored[199]
    genes, F = population(eng, sp.B, P)
    want = expected(genes, F)
    got = front(eng, sp.B, P)
    check_front(got, want, "k_last")
    for b, prob in enumerate(sy.probs):
        gl, gu = mo.genetic_bounds(sy.lay, prob.xl, prob.xu)
        assert gl[199] == gu[199]
        assert (genes[b][:, 199] == gl[199]).all()
        assert (got[2][want[1][b]:want[1][b + 1], 199] == gl[199]).all()
    assert report("k_last", want[0], genes)[1] == sp.B
    monkeypatch.setenv("MV_COMPACT", "0")
    full = attack(sy, P, O, G)
    assert full.stored_genes().all()
    g0, F0 = population(full, sp.B, P)
    np.testing.assert_array_equal(genes, g0)
    # the compact layout folds the fixed gene's layer-0 term into the state's bias: f1 is
    # another fp32 sum (the suite's classifier tolerance), f2 and f3 are the same numbers
    np.testing.assert_array_equal(F[..., 1:], F0[..., 1:])
    np.testing.assert_allclose(F[..., 0], F0[..., 0], rtol=1e-5, atol=1e-7)
    check_front(front(full, sp.B, P), expected(g0, F0), "k_last under MV_COMPACT=0")


@pytest.mark.parametrize("B,G", [(1025, 2), (2500, 2), (1025, 30), (2500, 30)])
def test_front_many_states(built, B, G):
    """More states than k_front_scan has threads: runs of 2 (B 1025: threads 513.. own no
    state) and 3 (B 2500: thread 833 owns one, 834.. none) states per thread.  Every state
    draws from its own random stream, so the populations differ.  At G 2 the population is
    chosen from 5 copies of the initial state and 4 offspring: its first front holds the 5
    copies, so no member can be dominated; at G 30 a few states end with one (streams 17 and
    230 on the oracle) and the front sizes differ."""
    P, O = 5, 4
    sy = built("n8p")
    eng = attack(sy, P, O, G, B=B, first=0)
    genes, F = population(eng, B, P)
    want = expected(genes, F)
    check_front(front(eng, B, P), want, f"B {B} (states 0, 1023, 1024 and {B - 1} included)")
    partial, moved = report(f"B {B} G {G}", want[0], genes)
    assert moved > B // 4
    assert len({genes[b].tobytes() for b in range(0, B, sp.B)}) > B // 12
    if G == 2:
        assert partial == 0
    else:
        assert not want[0][17].all() and not want[0][230].all() and partial >= 2


# ------------------------------------------------------------------ the kernels on any F
def synthetic_F(B, P, rng):
    """Populations with every kind of row the relation meets, one kind per state in turn:
    0: objectives on a grid of 4 values (ties in every objective, duplicates, a small front);
    1: continuous values (a front of a tenth of the members or so, scattered over the
       population) with an infinite, a NaN and a -0.0 / 0.0 pair among them;
    2: one row repeated (identical rows do not dominate each other: all front);
    3: a chain, every member dominated by the next: the front is the last member alone."""
    F = np.empty((B, P, 3))
    for b in range(B):
        kind = b % 4
        if kind == 0:
            F[b] = rng.integers(0, 4, (P, 3))
        elif kind == 1:
            F[b] = rng.standard_normal((P, 3))
            F[b, rng.integers(0, P), 0] = np.inf
            F[b, rng.integers(0, P), 1] = np.nan
            if P > 1:
                F[b, 0], F[b, P - 1] = (0.0, -0.0, -3.0), (-0.0, 0.0, -3.0)
        elif kind == 2:
            F[b] = rng.standard_normal(3)
        else:
            F[b] = -np.arange(P)[:, None] * np.array([1.0, 0.0, 2.0]) + rng.standard_normal(3)
    return F


def run_front(F, genes, X=True, Fx=True):
    from moeva2_amd import _native

    B, P, V = genes.shape
    n = B * P + 1
    t = [torch.full((B, P), 7, dtype=torch.uint8, device="cuda"),
         torch.full((B + 1,), -1, dtype=torch.int32, device="cuda"),
         torch.full((n, V), float("nan"), dtype=torch.float64, device="cuda") if X else None,
         torch.full((n, 3), float("nan"), dtype=torch.float64, device="cuda") if Fx else None]
    _native.front(torch.as_tensor(F, device="cuda"), t[0], t[1],
                  genes=torch.as_tensor(genes, device="cuda") if X else None, X=t[2], Fx=t[3])
    torch.cuda.synchronize()
    return [None if v is None else v.cpu().numpy() for v in t]


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, P_MAX])
def test_front_kernels_on_any_F(P):
    """mv_front runs mv_attack_front's three kernels on a caller's F, so the relation and the
    compaction over excluded members are pinned on dominated rows at every population size."""
    B, V = 8, 5
    rng = np.random.default_rng(300 + P)
    F, genes = synthetic_F(B, P, rng), rng.standard_normal((B, P, V))
    want = expected(genes, F)
    nd = want[0]
    if P > 2:
        size = nd.sum(axis=1)
        assert (size[0::4] < P).all() and (size[1::4] < P).all() and (size[1::4] > 1).all()
        assert (size[2::4] == P).all() and (size[3::4] == 1).all() and nd[3, P - 1]
        # excluded members before, between and after the front's: ranks are not positions
        assert not nd[1, :P // 2].all() and nd[1, P // 2:].any() and not nd[1, P // 2:].all()
    got = run_front(F, genes)
    # NaN objectives are the sentinel's value too: compare Fx through the bit patterns
    check_front(got[:3] + [None], want, f"any F, P {P}")
    n = int(want[1][-1])
    np.testing.assert_array_equal(got[3][:n].view(np.int64), want[3].view(np.int64))
    assert np.isnan(got[3][n:]).all()
    check_front(run_front(F, genes, X=False, Fx=False), want, f"any F, P {P}, mask only")


@pytest.mark.parametrize("B", [1025, 2500])
def test_front_scan_on_uneven_fronts(B):
    """k_front_scan's runs of 2 and 3 states per thread over front sizes 1..5."""
    P, V = 5, 3
    rng = np.random.default_rng(B)
    F = rng.integers(0, 3, (B, P, 3)).astype(np.float64)
    genes = rng.standard_normal((B, P, V))
    want = expected(genes, F)
    assert set(np.diff(want[1])) == {1, 2, 3, 4, 5}
    check_front(run_front(F, genes), want, f"uneven fronts, B {B}")
