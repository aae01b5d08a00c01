"""The restatements the k_mlp and bf16 GPU tests compare against, checked without a GPU:
oracle/device_order's ``kernel="mlp_v1"`` order (tests/test_gpu_mlp_fallback.py), the bf16
rounding and the three accumulation variants of tests/bf16_ref.py
(tests/test_gpu_bf16_routes.py), and the fallback cases' lines of the route table."""
import re

import numpy as np
import pytest

import bf16_ref
import synth_problem as sp
from oracle import device_order as do
from oracle import moeva_oracle as mo
from test_routes_cpu import EXPECTED

DIMS = (47, 144, 80, 3)


@pytest.fixture(scope="module")
def small():
    """A 47-144-80-3 net over 47 features (every third immutable), 33 random rows."""
    rng = np.random.default_rng(5)
    D = DIMS[0]
    W, bs = sp.net(DIMS, 6)
    mutable = np.arange(D) % 3 != 2
    lay = mo.make_layout(mutable, np.array(["real"] * D, object))
    x0 = rng.uniform(0.0, 1.0, D)
    ml = (rng.uniform(0.5, 2.0, D), rng.uniform(-0.5, 0.5, D))
    prob = mo.make_problem(lay, x0, np.zeros(D), np.ones(D), ml, W, bs, None, 2, 2, True)
    x = np.tile(x0, (33, 1))
    x[:, mutable] = rng.uniform(0.0, 1.0, (33, int(mutable.sum())))
    return prob, x, W, bs, np.where(mutable)[0]


def _forward64(x_ml, W, bs):
    h = np.asarray(x_ml, np.float64).astype(np.float32).astype(np.float64)
    for i, (w, b) in enumerate(zip(W, bs)):
        h = h @ w.astype(np.float64) + b.astype(np.float64)
        if i + 1 < len(W):
            h = np.maximum(h, 0.0)
    e = np.exp(h - h.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def test_mlp_v1_order_is_a_forward_and_its_own_order(small):
    prob, x, W, bs, _ = small
    f = do.f1_device_order(prob, x, kernel="mlp_v1")
    ref = _forward64(x * prob.ml_scale + prob.ml_min, W, bs)[:, 2]
    np.testing.assert_allclose(f, ref, rtol=1e-5, atol=1e-7)
    # a GPU test cannot pass under the wrong order's name: the two orders differ in some bit
    assert (f != do.f1_device_order(prob, x, kernel="mlp2")).any()
    assert (f != do.f1_device_order(prob, x, kernel="mlpw32")).any()
    with pytest.raises(ValueError):
        do.f1_device_order(prob, x, kernel="mlp")


def test_bf16_rounding_equals_torch():
    torch = pytest.importorskip("torch")
    f = np.float32
    u = lambda bits: np.array(bits, np.uint32).view(np.float32)  # noqa: E731
    v = np.concatenate([
        u([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000]),  # ties: to even down, up, both signs
        u([0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001]),  # one fp32 ulp either side of a tie
        u([0x7F7FFFFF, 0xFF7FFFFF]),                          # largest finite: rounds to inf
        u([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001]),  # fp32 subnormals
        np.array([0.0, -0.0, np.inf, -np.inf], f),
        np.random.default_rng(1).standard_normal(64).astype(f)])
    got = bf16_ref.bf16(v)
    ref = torch.tensor(v).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.isinf(got[8]) and np.isinf(got[9]) and np.signbit(got[-64 - 3])
    assert got[0] == u([0x3F800000])[0] and got[1] == u([0x3F820000])[0]


def test_bf16_variants_agree(small):
    prob, x, W, bs, mut = small
    x_ml = x * prob.ml_scale + prob.ml_min
    P = {v: bf16_ref.bf16_forward(x_ml, mut, W, bs, v) for v in "ABC"}
    for v in "BC":
        np.testing.assert_allclose(P[v], P["A"], rtol=0, atol=1e-3)
    # the bf16 arithmetic is not the fp32 one (it would pass a test of either otherwise)
    assert np.abs(P["A"] - _forward64(x_ml, W, bs)).max() > 1e-5
    f, floor = bf16_ref.f1_with_floor(x_ml, mut, W, bs, 2)
    np.testing.assert_array_equal(f, P["A"][:, 2])
    assert bf16_ref.FLOOR_MIN <= floor < 1e-3


# ------------------------------------------------------------------ the fallback cases' routes
_KIND = {0: "k_mlp", 1: "k_mlp2(genes)", 4: "k_mlpw", 5: "k_mlpw32"}
_LINE = re.compile(r"mlp synth (\S+) Dm4 (\d+) (\S+) (fp32|bf16)( MV_MLP_V1)?\s+kind=(-?\d+) .* "
                   r"bf=(\d) .* maxct=(\d)$")
# (case, mode) -> (kind, maxct): the instance each GPU case names
INSTANCES = {
    ("m608w", "fp32"): ("k_mlpw32", 0), ("m609w", "fp32"): ("k_mlp", 8),
    ("m736w", "fp32"): ("k_mlp", 8), ("m1008w", "fp32"): ("k_mlp", 4),
    ("m640n", "fp32"): ("k_mlp2(genes)", 0), ("m640n", "fp32 MV_MLP_V1"): ("k_mlp", 2),
    ("m639t", "fp32"): ("k_mlp2(genes)", 0), ("m639t", "fp32 MV_MLP_V1"): ("k_mlp", 1),
    ("m609w", "bf16"): ("k_mlp", 8), ("m1008w", "bf16"): ("k_mlp", 4),
}


def _lines():
    out = {}
    for line in EXPECTED.splitlines():
        m = _LINE.match(line)
        if m:
            name, dm4, net, mode, v1, kind, bf, maxct = m.groups()
            out[name, mode + (v1 or "")] = (int(dm4), net, _KIND[int(kind)], int(bf), int(maxct))
    return out


@pytest.mark.parametrize("name,mode", sorted(INSTANCES), ids=lambda v: v.replace(" ", "-"))
def test_route_table_pins_the_fallback_case(name, mode):
    """The case's line of the route table was computed for the case's shape and net, and gives
    the kernel and the MAXCT / BF instance the GPU tests name."""
    case = sp.MLP_BY_NAME[name]
    dm4, net, kind, bf, maxct = _lines()[name, mode]
    assert dm4 == (case.Dm + 15) // 16 * 16 and net == "-".join(map(str, case.net))
    assert (kind, maxct) == INSTANCES[name, mode] and bf == int(mode == "bf16")
    if mode == "fp32":
        assert kind == case.mlp
    elif mode == "fp32 MV_MLP_V1":
        assert kind == case.mlp_v1


def test_every_fallback_instance_has_a_line():
    got = {(v[3], v[4]) for v in _lines().values() if v[2] == "k_mlp"}
    assert got >= {(0, 1), (0, 2), (0, 4), (0, 8), (1, 4), (1, 8)}
    assert set(k[0] for k in _lines()) == set(sp.MLP_BY_NAME)
