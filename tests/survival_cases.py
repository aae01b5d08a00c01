"""Survival inputs at k_survive's fallback branches and size edges (helper module, not a test
file), with a witness of the branch every state took.

A ``Case`` holds the merged objective arrays of 2-3 generations for B >= 3 states of
*different* data (a row read from another state's buffer shows up), the reference points and
``n_survive``; the carried state (ideal, worst, extreme points) runs through the generations, so
``has_extreme`` and the previous extremes are live from the second one on.  ``oracle_run(case)``
runs ``mo.survive`` once per case (cached: the CPU witness test and the GPU comparison share it)
and returns, per generation and state, the oracle's result, the carried state after the call
and ``witness(...)``.

``witness`` re-derives in plain numpy, from the oracle's own intermediates, which branch of
csrc/survival.h the state takes:

  nadir        'singular' (a zero pivot: np.linalg.solve's LinAlgError) | 'notclose' (the plane
               does not reproduce the extreme points) | 'small' (an intercept <= 1e-6) | 'plane'
  clampworst   'plane' and a component of ideal + intercepts above the carried worst point
  wfront       a nadir component within 1e-6 of the ideal point, replaced by the front's worst
  den0         a zero nadir - ideal component in the association (-> 1e-12)
  dotsmall     reference points whose |dot| <= 1e-6 in the line / plane intersection
  clamp        aspiration directions with a non-positive component (the res < 0 clamp)
  at_ideal     ranked rows exactly at the ideal point (normalised objectives all +0)
  nonfinite    ranked rows with a non-finite normalised objective
  ovf          ranked rows whose exact distance is attained by more than four directions of
               one half of the two-lane sweep (the wave-parallel exact pass)
  ovf5         the same with exactly five in a half (and no half above five)
  fronts, n_ranked, niching, max_niche_last (largest number of last-front members in a niche)

Every case carries ``expect``: the witness values it is built for, asserted for every state by
tests/test_survival_edges_cpu.py on the oracle alone and again by the GPU test, so a case
cannot drift off its branch silently.
"""
import dataclasses
import functools
from typing import Dict, List

import numpy as np

from oracle import moeva_oracle as mo
from moeva2_amd.attacks.moeva2.ref_dirs import energy_ref_dirs

B = 3  # states per case
MU = 0.05
ASP = np.full((1, 3), 1.0 / 3.0)
ONE = np.array([[1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]])

# csrc/engine.h, csrc/survival.h
SURV_NLDS, SURV_NMAX, SURV_RMAX, NICHE_SORT_MIN = 512, 1024, 640, 256


@dataclasses.dataclass
class Case:
    name: str
    F: List[np.ndarray]  # per generation (B, N, 3)
    ref: np.ndarray      # (R, 3)
    n_survive: int
    expect: List[Dict]   # per generation: witness key -> value, or a predicate of the value
    seed: int = 42

    @property
    def N(self):
        return self.F[0].shape[1]

    @property
    def R(self):
        return self.ref.shape[0]


def _align16(x):
    return (x + 15) & ~15


def alias_of(N, R):
    """surv_offsets' ``alias``: the niching temporaries lie inside the dominance bitsets
    (tests/native/surv_offsets_check.cpp prints the header's own value; the CPU test compares)."""
    RN, NW = R + 3, (N + 63) // 64
    t = 0
    for b in (RN * 4, RN * 4, (RN + 1) * 4, N * 4, RN * 4, RN * 4, RN * 8, (2 * N + 2) * 4):
        t = _align16(t + b)
    return int(N <= SURV_NLDS and t <= N * NW * 8)


def sweep_residues(R):
    """(RN parity, nh & 3, n4 & 3) of the two-lane association sweep (survival.h)."""
    RN = R + 3
    nh = RN >> 1
    return ("odd" if RN & 1 else "even"), nh & 3, (nh >> 2) & 3


# ------------------------------------------------------------------------------- witness
def witness(F, n_survive, ideal, worst, extreme, r, ref, mu=MU):
    """Branches of one survival call: ideal / worst / extreme are the carried state *after*
    the call (what the nadir is computed from), r the oracle's SurvivalResult."""
    w = {}
    M = extreme - ideal
    with np.errstate(all="ignore"):
        pl = mo.lu_solve3(M, np.ones(3))
        wpop = np.max(F, axis=0)
        if pl is None:
            w["nadir"], pre = "singular", wpop
        else:
            ic = 1.0 / pl
            Mp = np.array([(M[i, 0] * pl[0] + M[i, 1] * pl[1]) + M[i, 2] * pl[2]
                           for i in range(3)])
            if not np.all(np.abs(Mp - 1.0) <= 1e-8 + 1e-5):
                w["nadir"], pre = "notclose", wpop
            elif np.any(ic <= 1e-6):
                w["nadir"], pre = "small", wpop
            else:
                w["nadir"] = "plane"
                pre = np.where(ideal + ic > worst, worst, ideal + ic)
        w["clampworst"] = bool(w["nadir"] == "plane" and np.any(ideal + ic > worst))
        w["wfront"] = bool(np.any(pre - ideal <= 1e-6))
        den = r.nadir - ideal
        w["den0"] = bool(np.any(den == 0))
        # the aspiration directions, as rnsga3.get_ref_dirs_from_points computes them
        nv = np.ones(3) / np.sqrt(3)
        l = (ref - ideal) / den
        dot = (l[:, 0] * nv[0] + l[:, 1] * nv[1]) + l[:, 2] * nv[2]
        big = np.abs(dot) > 1e-6
        w["dotsmall"] = int((~big).sum())
        wn = (1.0 * nv[0] + 0.0 * nv[1]) + 0.0 * nv[2]
        ia = 0.0 + l * (wn / dot)[:, None]
        q = l - np.eye(3)[0]
        t = (q[:, 0] * nv[0] + q[:, 1] * nv[1]) + q[:, 2] * nv[2]
        ib = l - t[:, None] * nv
        res = (mu * ASP[0])[None, :] + (np.where(big[:, None], ia, ib) - (mu * ASP[0])[None, :])
        fix = ~(res > 0).min(axis=1)
        w["clamp"] = int(fix.sum())
        rf = res[fix]
        rf[rf < 0] = 0
        res[fix] = rf / ((rf[:, 0] + rf[:, 1]) + rf[:, 2])[:, None]
        np.testing.assert_array_equal(np.concatenate([res, np.eye(3)]), r.ref_dirs)
        # association
        I = np.concatenate(r.fronts)
        Nn = (F[I] - ideal) / np.where(den == 0, 1e-12, den)
        w["at_ideal"] = int(np.sum(np.all((Nn == 0) & ~np.signbit(Nn), axis=1)))
        w["nonfinite"] = int(np.sum(~np.isfinite(Nn).all(axis=1)))
        U = mo.normalized_dirs(r.ref_dirs)
        s = (Nn[:, None, 0] * U[None, :, 0] + Nn[:, None, 1] * U[None, :, 1]) \
            + Nn[:, None, 2] * U[None, :, 2]
        e = [s * U[None, :, k] - Nn[:, None, k] for k in range(3)]
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        np.testing.assert_array_equal(dist[np.arange(len(I)), r.niche], r.dist)
        tie = dist == r.dist[:, None]
        nh = (len(U)) >> 1
        per_half = np.stack([tie[:, :nh].sum(axis=1), tie[:, nh:].sum(axis=1)], axis=1)
        w["ovf"] = int(np.sum(per_half.max(axis=1) > 4))
        w["ovf5"] = int(np.sum(per_half.max(axis=1) == 5))
    w["fronts"] = len(r.fronts)
    w["n_ranked"] = len(I)
    w["niching"] = bool(len(I) > n_survive)
    last = r.niche[len(I) - len(r.fronts[-1]):]
    w["max_niche_last"] = int(np.bincount(last).max())
    return w


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    case = CASES[name]()
    out = []
    st = [mo.SurvivalState() for _ in range(case.F[0].shape[0])]
    for gen, F in enumerate(case.F):
        row = []
        for b in range(F.shape[0]):
            r = mo.survive(F[b], case.n_survive, st[b], case.ref, ASP, MU, case.seed, gen)
            snap = (st[b].ideal.copy(), st[b].worst.copy(), st[b].extreme.copy())
            row.append((r, snap, witness(F[b], case.n_survive, *snap, r, case.ref)))
        out.append(row)
    for a in case.F + [case.ref]:
        a.setflags(write=False)
    return case, out


def oracle_run(name):
    """(case, [generation][state] -> (SurvivalResult, (ideal, worst, extreme), witness))."""
    return _oracle_run(name)


def check_witness(case, out):
    """Every state of every generation took the branches the case was built for."""
    assert len(case.expect) == len(case.F)
    for gen, (row, exp) in enumerate(zip(out, case.expect)):
        for b, (_r, _s, w) in enumerate(row):
            for k, v in exp.items():
                ok = v(w[k]) if callable(v) else w[k] == v
                assert ok, f"{case.name} gen {gen} state {b}: witness {k} = {w[k]!r} ({w})"


# ------------------------------------------------------------------------------- inputs
def random_F(rng, n_states, N, lo=0.0, hi=1.0):
    """Uniform rows with ties in f1, duplicated rows and zeros in f3 (as the parity tests')."""
    F = np.empty((n_states, N, 3))
    for b in range(n_states):
        f = rng.uniform(lo, hi, size=(N, 3))
        f[:, 0] = np.round(f[:, 0], 2)
        f[: N // 10] = f[N // 10: 2 * (N // 10)]
        if N >= 10:
            f[-5:, 2] = lo
        F[b] = f
    return F


@functools.lru_cache(maxsize=None)
def _simplex_refs(R, seed):
    if R >= 3:
        X = energy_ref_dirs(3, R, seed=seed)
        if X.shape[0] == R:
            return X
    return np.random.default_rng(1000 + R).dirichlet(np.ones(3) * 2.0, size=R)


def simplex_refs(R, seed=1):
    """energy_ref_dirs where it returns exactly R points (it holds the three corners, so it
    returns 3 below that), else seeded points inside the simplex."""
    return _simplex_refs(R, seed).copy()


def _ns(N):
    return max(1, (2 * N) // 3)


CASES = {}


def _case(name):
    def reg(fn):
        CASES[name] = lambda: fn(name)
        return fn
    return reg


gt0 = lambda v: v > 0  # noqa: E731


def _planted(rng, N, gen, rows, lo, hi):
    """(B, N, 3): uniform rows in [lo, hi] s with the three given rows (times s) planted at
    positions that differ by state and generation; s = 1 + b / 4 is the state's scale (the
    same in every generation, so the planted rows stay the extreme points)."""
    F = np.empty((B, N, 3))
    for b in range(B):
        sc = 1.0 + 0.25 * b
        F[b] = rng.uniform(lo, hi, size=(N, 3)) * sc
        at = (np.array([1, 17, 30]) + 3 * b + gen) % N
        F[b, at] = np.array(rows, np.float64) * sc
    return F


def _branch_cases(N):
    tag = f"N{N}"

    @_case(f"singular_den0_wfront-{tag}")
    def _(name):
        """R 1, the even rows clones of c = (0.5, 0.2, 0.1) s and the odd rows clones of
        (0.6, 0.25, 0.1 + 5e-7) s, which c dominates: two of the three extreme points are the
        same row, the nadir falls to the population's worst, whose third component lies within
        1e-6 of the ideal point and is replaced by the front's worst (another value: 0.1 s),
        and the association divides by 1e-12.  The zero width makes the reference direction
        NaN, so np.argmin gives every row direction 0 at a NaN distance."""
        F = []
        for g in range(3):
            f = np.empty((B, N, 3))
            for b in range(B):
                sc = (1.0 + 0.25 * b) * (1.0 - 0.125 * g)
                f[b, 0::2] = np.array([0.5, 0.2, 0.1]) * sc
                f[b, 1::2] = np.array([0.6, 0.25, 0.1 + 5e-7]) * sc
            F.append(f)
        e = dict(nadir="singular", wfront=True, den0=True, fronts=2, n_ranked=N, niching=False)
        return Case(name, F, ONE.copy(), N, [e, e, e])

    @_case(f"plane_clampworst-{tag}")
    def _(name):
        """R 1 at the simplex centre; the extreme points are three planted rows (s, 0, 0),
        (0, s, 0.0009 s), (0, 0, s) (every other row is far from the axes), whose plane meets
        axis 2 at 1.0009 s, above the worst point's s.  The one aspiration direction is
        interior (the res < 0 clamp stays off)."""
        rng = np.random.default_rng(N + 1)
        F = [_planted(rng, N, g, [[1, 0, 0], [0, 1, 0.0009], [0, 0, 1]], 0.2, 0.9)
             for g in range(3)]
        e = dict(nadir="plane", clampworst=True, wfront=False, den0=False, clamp=0, dotsmall=0)
        return Case(name, F, ONE.copy(), _ns(N), [e, e, e])

    @_case(f"plane-{tag}")
    def _(name):
        """The benign branch, for the contrast: energy reference points (corners included, so
        the direction clamp is on)."""
        rng = np.random.default_rng(N + 2)
        F = [random_F(rng, B, N) for _ in range(2)]
        e = dict(nadir="plane", clampworst=False, wfront=False, den0=False, clamp=gt0,
                 dotsmall=0)
        return Case(name, F, energy_ref_dirs(3, 200, seed=1), _ns(N), [e, e])

    @_case(f"singular_dotsmall-{tag}")
    def _(name):
        """One reference point below every row: it is the ideal point, every extreme point and
        a direction with dot == 0."""
        rng = np.random.default_rng(N + 3)
        F = [random_F(rng, B, N, 0.5, 1.0) for _ in range(3)]
        e = dict(nadir="singular", dotsmall=1)
        return Case(name, F, np.array([[0.1, 0.1, 0.1]]), _ns(N), [e, e, e])

    @_case(f"small-{tag}")
    def _(name):
        """A negative intercept: the extreme points are three planted rows (s, 0, 0),
        (0.5 s, 0.1 s, 0.8 s), (0, 0, s) (every other row and both reference points are
        farther from axis 2 than the second one), whose plane meets axis 2 at -s / 3."""
        rng = np.random.default_rng(N + 4)
        F = [_planted(rng, N, g, [[1, 0, 0], [0.5, 0.1, 0.8], [0, 0, 1]], 0.85, 0.95)
             for g in range(3)]
        ref = np.array([[0.9] * 3, [0.95] * 3])
        e = dict(nadir="small", den0=False)
        return Case(name, F, ref, _ns(N), [e, e, e])

    @_case(f"at_ideal-{tag}")
    def _(name):
        """One row exactly at the ideal point (the origin, with the corners' zeros)."""
        rng = np.random.default_rng(N + 5)
        F = [random_F(rng, B, N) for _ in range(2)]
        for g, f in enumerate(F):
            for b in range(B):
                f[b, (7 + 3 * b + g) % N] = 0.0
        e = dict(at_ideal=1, n_ranked=N)
        return Case(name, F, simplex_refs(20), N, [e, e])

    @_case(f"ovf_repeat6-{tag}")
    def _(name):
        """Each of 10 reference points 6 times: every ranked row ties over six directions."""
        rng = np.random.default_rng(N + 6)
        F = [random_F(rng, B, N) for _ in range(2)]
        ref = np.repeat(simplex_refs(10), 6, axis=0)
        e = dict(ovf=gt0)
        return Case(name, F, ref, _ns(N), [e, e])

    @_case(f"ovf_five-{tag}")
    def _(name):
        """Interior reference points, each at five scattered positions (3, 4, 5, 6, 8 of a
        block of 10: the lowest index is the fifth hit in the sweep's chain order), so a half
        of the sweep holds exactly five tied directions."""
        rng = np.random.default_rng(N + 7)
        F = [random_F(rng, B, N) for _ in range(2)]
        pts = np.random.default_rng(77).dirichlet(np.ones(3) * 3.0, size=8)
        ref = np.empty((40, 3))
        for blk in range(4):
            fill = [0, 1, 2, 7, 9]
            ref[blk * 10 + np.array([3, 4, 5, 6, 8])] = pts[2 * blk]
            ref[blk * 10 + np.array(fill)] = pts[2 * blk + 1]
        e = dict(ovf5=gt0)
        return Case(name, F, ref, _ns(N), [e, e])

    @_case(f"inf-{tag}")
    def _(name):
        """One +inf objective in a non-dominated row (its f1 below every other row's)."""
        rng = np.random.default_rng(N + 8)
        F = [random_F(rng, B, N) for _ in range(3)]
        for g, f in enumerate(F):
            for b in range(B):
                i = (3 + 5 * b + g) % N
                f[b, i] = [-1.0 - b - g, np.inf, 0.5]
        e = dict(nonfinite=gt0)
        return Case(name, F, simplex_refs(20), _ns(N), [e, e, e])

    @_case(f"nan-{tag}")
    def _(name):
        """One NaN objective: the ideal point's component is NaN from then on."""
        rng = np.random.default_rng(N + 9)
        F = [random_F(rng, B, N) for _ in range(3)]
        for b in range(B):
            F[0][b, (3 + 5 * b) % N, 1] = np.nan
        e = dict(nadir="notclose", nonfinite=gt0)
        return Case(name, F, simplex_refs(20), _ns(N), [e, e, e])


BRANCH_N = (40, 303, 600)
for _N in BRANCH_N:
    _branch_cases(_N)
BRANCH_CASES = [n for n in CASES]

# ---- R edges (N 120)
R_EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 14, 17, 22, 27, 61, 62, 63, 64, 65, 640)


def r_edge_id(R):
    par, a, c = sweep_residues(R)
    return f"R{R}-RN{par}-nh&3={a}-n4&3={c}"


def _r_edge(R):
    @_case(r_edge_id(R))
    def _(name):
        rng = np.random.default_rng(5000 + R)
        F = [random_F(rng, B, 120) for _ in range(2)]
        e = dict(n_ranked=lambda v: v >= 80, nonfinite=0, den0=False)
        return Case(name, F, simplex_refs(R), 80, [e, e])


for _R in R_EDGES:
    _r_edge(_R)
R_EDGE_CASES = [r_edge_id(R) for R in R_EDGES]

# ---- N edges (R 20 and R 200)
N_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)


def n_edge_id(N, R):
    return f"N{N}-R{R}-alias{alias_of(N, R)}"


def _n_edge(N, R):
    @_case(n_edge_id(N, R))
    def _(name):
        rng = np.random.default_rng(7000 + N + R)
        F = [random_F(rng, B, N) for _ in range(2)]
        e = dict(n_ranked=lambda v: v >= _ns(N), nonfinite=0, den0=False)
        return Case(name, F, simplex_refs(R), _ns(N), [e, e])


for _R in (20, 200):
    for _N in N_EDGES:
        _n_edge(_N, _R)
_n_edge(1024, 640)
N_EDGE_CASES = [n_edge_id(N, R) for R in (20, 200) for N in N_EDGES]
N1024_R640 = n_edge_id(1024, 640)


# ---- n_survive edges: K mutually non-dominated rows per front, LAYERS fronts
K_FRONT, LAYERS = 20, 6


def _layered(rng):
    F = np.empty((B, K_FRONT * LAYERS, 3))
    for b in range(B):
        S = rng.dirichlet(np.ones(3), size=K_FRONT) * (1.0 + 0.5 * b)
        rows = np.concatenate([S + 0.25 * f for f in range(LAYERS)])
        F[b] = rows[rng.permutation(len(rows))]
    return F


def _n_survive_case(tag, n_survive, expect):
    @_case(f"layered-{tag}")
    def _(name):
        rng = np.random.default_rng(9000)
        F = [_layered(rng) for _ in range(2)]
        return Case(name, F, simplex_refs(20), n_survive, [expect, expect])


_NL = K_FRONT * LAYERS
_n_survive_case("n_survive1", 1, dict(fronts=1, n_ranked=K_FRONT, niching=True))
_n_survive_case("n_surviveN", _NL, dict(fronts=LAYERS, n_ranked=_NL, niching=False))
_n_survive_case("boundary", 2 * K_FRONT, dict(fronts=2, n_ranked=2 * K_FRONT, niching=False))
_n_survive_case("boundary+1", 2 * K_FRONT + 1,
                dict(fronts=3, n_ranked=3 * K_FRONT, niching=True))


def _chain(N):
    @_case(f"chain-N{N}")
    def _(name):
        """Row i = (i, i, i) (scaled and permuted per state): N fronts of one row each."""
        rng = np.random.default_rng(N)
        F = []
        for g in range(2):
            f = np.empty((B, N, 3))
            for b in range(B):
                f[b] = (rng.permutation(N)[:, None] * np.ones((1, 3))) * (1.0 + b + 0.5 * g)
            F.append(f)
        e = dict(fronts=N, n_ranked=N, niching=False, at_ideal=1)
        return Case(name, F, simplex_refs(20), N, [e, e])


_chain(65)
_chain(1024)
N_SURVIVE_CASES = ["layered-n_survive1", "layered-n_surviveN", "layered-boundary",
                   "layered-boundary+1", "chain-N65", "chain-N1024"]


# ---- niche sort switch: one front on a plane, the fullest niche at 256 | 257 members
def _plane_rows(rng, n):
    w = rng.dirichlet(np.ones(3) * 1.5, size=n)
    f = np.round(w, 4)
    f[:, 2] = 1.0 - f[:, 0] - f[:, 1]
    return f


def _niche_F(rng, N, full, scale, F0):
    """N rows on the plane f1 + f2 + f3 = scale for the generation after F0, one point
    repeated until the fullest niche of the (single) front holds exactly ``full`` members."""
    ref = simplex_refs(20)
    st0 = mo.SurvivalState()
    mo.survive(F0, _ns(N), st0, ref, ASP, MU, 42, 0)
    others = _plane_rows(rng, N) * scale
    p = np.array([0.3125, 0.375, 0.3125]) * scale
    k = full
    for _ in range(20):
        F = np.concatenate([np.tile(p, (k, 1)), others[: N - k]])
        st = mo.SurvivalState(st0.ideal.copy(), st0.worst.copy(), st0.extreme.copy())
        r = mo.survive(F, _ns(N), st, ref, ASP, MU, 42, 1)
        m = int(np.bincount(r.niche).max())
        if m == full:
            return F[rng.permutation(N)]
        k += full - m
    raise AssertionError("no fixed point for the niche size")


def _niche_case(N, full):
    @_case(f"niche{full}-N{N}")
    def _(name):
        rng = np.random.default_rng(N + full)
        F0 = np.stack([_plane_rows(rng, N) * (1.0 + 0.5 * b) for b in range(B)])
        F1 = np.stack([_niche_F(rng, N, full, 1.0 + 0.5 * b, F0[b]) for b in range(B)])
        e0 = dict(fronts=1, n_ranked=N, niching=True,
                  max_niche_last=lambda v: v < NICHE_SORT_MIN)
        e1 = dict(fronts=1, n_ranked=N, niching=True, max_niche_last=full)
        return Case(name, [F0, F1], simplex_refs(20), _ns(N), [e0, e1])


for _N in (512, 600, 1024):
    for _full in (NICHE_SORT_MIN, NICHE_SORT_MIN + 1):
        _niche_case(_N, _full)
NICHE_CASES = [f"niche{f}-N{N}" for N in (512, 600, 1024)
               for f in (NICHE_SORT_MIN, NICHE_SORT_MIN + 1)]

ALL_CASES = list(CASES)
