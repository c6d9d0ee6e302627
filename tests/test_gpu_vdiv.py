"""The device's division of a vector by one scalar (dt_math.h divs_shared: one reciprocal refinement
for the three quotients where their scaled divisors are bitwise equal, three plain divisions in a
branch elsewhere) against three plain divisions on the device, bit for bit, and both against numpy's
correctly rounded float64 a / s and a / sqrt((x*x + y*y) + z*z). One array, one launch
(dt_debug_vdiv), shared by the tests below: ordinary vectors, vectors and divisors with exponents
from the whole double range, and hand-written edge cases, mixed within the 64-lane waves."""
import numpy as np
import pytest

import distraytracer_amd as dt

pytestmark = pytest.mark.gpu

INF, NAN = np.inf, np.nan
SUB = 5e-324          # the smallest subnormal
HAND = [  # (x, y, z, divisor)
    (0.0, 1.0, 2.0, 3.0), (-0.0, 1.0, 2.0, 3.0), (0.0, -0.0, 5.0, -7.0), (-0.0, -0.0, -3.0, 0.5),
    (0.0, 0.0, 0.0, 2.0), (-0.0, 0.0, -0.0, 2.0), (0.0, 0.0, 0.0, 0.0),           # all zero: normalized returns them
    (SUB, 1.0, 2.0, 3.0), (1e-310, -2e-320, SUB, 1.5), (1.0, 2.0, 3.0, 1e-310), (1.0, 2.0, 3.0, SUB),
    (1e-310, 1e-310, 1e-310, 1e-310), (SUB, SUB, SUB, 3.0),
    (1e300, 1e300, 1e300, 1e-300), (1e-300, 1e-300, 1e-300, 1e300),
    (1e300, 1.0, 1.0, 1e-300), (1.0, 1e-300, 1.0, 1e300), (1e300, 1e-300, 1.0, 1.0), (1.0, 1.0, 1e-300, 1e300),
    (2.0 ** 1000, 2.0 ** -1000, 1.0, 3.0), (2.0 ** -600, 2.0 ** -600, 0.0, 2.0 ** 600),
    (INF, 1.0, 2.0, 3.0), (-INF, 1.0, 2.0, 3.0), (1.0, INF, -INF, INF), (1.0, 2.0, 3.0, INF), (1.0, 2.0, 3.0, -INF),
    (NAN, 1.0, 2.0, 3.0), (1.0, 2.0, NAN, 3.0), (1.0, 2.0, 3.0, NAN), (INF, NAN, 0.0, 0.0), (1.0, -2.0, 3.0, 0.0),
    (1.0, -2.0, 3.0, -0.0),
    (3.0, 4.0, 5.0, 3.0), (3.0, 4.0, 5.0, 4.0), (0.1, 0.2, 0.3, 0.3), (-7.5, 7.5, 1.0, 7.5),   # divisor = a component
    (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 2.0), (0.0, 0.0, 1.0, 0.1), (-1.0, 0.0, 0.0, 3.0), (0.0, -1.0, -0.0, 1.0),
    (-0.0, 0.0, -1.0, 7.0), (3.0, 4.0, 0.0, 5.0), (1e200, 1e200, 1.0, 1e200), (1e-160, 0.0, 0.0, 1e-160),
]
N_ORDINARY, N_WILD, N_PURE = 49152, 16384, 8192


def _random_doubles(rng, shape):
    """sign, exponent field (1..2046: every normal binade) and fraction drawn independently"""
    bits = (rng.integers(0, 2, size=shape, dtype=np.uint64) << np.uint64(63)
            | rng.integers(1, 2047, size=shape, dtype=np.uint64) << np.uint64(52)
            | rng.integers(0, 1 << 52, size=shape, dtype=np.uint64))
    return bits.view(np.float64)


def _inputs():
    rng = np.random.default_rng(20)
    d = rng.normal(size=(N_ORDINARY, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    ordinary = d * 10.0 ** rng.uniform(-3, 3, size=(N_ORDINARY, 1))
    ordinary_s = 10.0 ** rng.uniform(-3, 3, size=N_ORDINARY) * rng.choice([-1.0, 1.0], size=N_ORDINARY)
    wild, wild_s = _random_doubles(rng, (N_WILD, 3)), _random_doubles(rng, N_WILD)
    hand = np.array(HAND * 5)   # (5 copies: the shuffle below drops them into several waves)
    # the first N_PURE vectors: waves of ordinary vectors only; behind them ordinary, wild and hand-written
    # ones shuffled, so a wave's lanes take both branches; 65536 + 225 vectors, 225 = 3 * 64 + 33
    v = np.concatenate([ordinary[N_PURE:], wild, hand[:, :3]])
    s = np.concatenate([ordinary_s[N_PURE:], wild_s, hand[:, 3]])
    p = rng.permutation(len(v))
    v, s = np.concatenate([ordinary[:N_PURE], v[p]]), np.concatenate([ordinary_s[:N_PURE], s[p]])
    assert len(v) % 64 == 33 and len(v) == 65536 + len(hand)
    return np.ascontiguousarray(v), np.ascontiguousarray(s)


@pytest.fixture(scope="module")
def run(cuda):
    v, s = _inputs()
    with np.errstate(all="ignore"):
        ref_div = v / s[:, None]
        n = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        ref_nrm = v.copy()
        pos = n > 0
        ref_nrm[pos] = v[pos] / np.sqrt(n[pos])[:, None]
    got = dt.debug_vdiv(v, s)
    for a in (ref_div, ref_nrm, v, s):
        a.setflags(write=False)
    return {"v": v, "s": s, "ref_divs": ref_div, "ref_normalized": ref_nrm, "got": got}


def _first(bad, run, a, b):
    i = int(np.argmax(bad.any(axis=1)))
    return "%d differ; first: %r / %r -> %r vs %r" % (bad.any(axis=1).sum(), run["v"][i], run["s"][i], a[i], b[i])


@pytest.mark.parametrize("what", ["divs", "normalized"])
def test_shared_equals_plain_bit_for_bit(run, what):
    """NaNs included, by payload: the shared path is the plain division's instructions on its operands"""
    a, b = run["got"][what + "_shared"], run["got"][what + "_plain"]
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), _first(bad, run, a, b)


@pytest.mark.parametrize("what", ["divs", "normalized"])
@pytest.mark.parametrize("path", ["shared", "plain"])
def test_equals_numpy(run, what, path):
    """correctly rounded: numpy's float64 quotient bit for bit (a NaN for a NaN: the host's payload differs)"""
    a, b = run["got"][what + "_" + path], run["ref_" + what]
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), _first(bad, run, a, b)


def test_both_paths_ran(run):
    """some vectors' scaled divisors differ (the plain branch ran), most vectors' do not (the shared one did)"""
    n = len(run["v"])
    fb = run["got"]["fallback_divs"]
    print("fallback: divs %d, normalized %d of %d" % (fb, run["got"]["fallback_normalized"], n))
    assert 0 < fb < n
    assert run["got"]["fallback_normalized"] < n
