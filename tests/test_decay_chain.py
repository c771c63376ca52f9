"""The decay chain (gsx_ops.h): k pending decays as k multiplies and ONE zero
test give, bit for bit, what k times "multiply, then test" gives, for
0 < d < 1 and 0 < DecayToZero.  numpy float64 on the CPU: IEEE multiplies and
compares, the operations of the kernels (built with -ffp-contract=off).

Compared for k = 0 .. 16 over random values, values that cross DecayToZero at
every step of the k, the special values, and decays from the spam-test
parameters and from the edges of (0, 1).  Outside the preconditions the two
forms differ (the last test): there the kernels keep the stepwise form."""
import numpy as np
import pytest

from gsx import synth

KS = range(17)
ULPS = (-3, -2, -1, 0, 1, 2, 3)


def stepwise(x, d, dtz, k):
    x = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for _ in range(k):
            x = x * np.float64(d)
            x = np.where(x < dtz, 0.0, x)
    return x


def chain(x, d, dtz, k):
    x = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for _ in range(k):
            x = x * np.float64(d)
        if k:  # k == 0: the input untouched, no test
            x = np.where(x < dtz, 0.0, x)
    return x


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ulps(x, n):
    """x moved by n units in the last place (x > 0 finite)."""
    return (np.array(x, dtype=np.float64).view(np.int64) + n).view(np.float64)


def decays():
    tp = synth.spam_test_topic_params()
    d7 = synth.bench_peer_params().behaviour_penalty_decay
    spam = [tp.first_message_deliveries_decay, tp.mesh_message_deliveries_decay, tp.mesh_failure_penalty_decay,
            tp.invalid_message_deliveries_decay, d7]
    edges = [np.nextafter(0.0, 1.0), 1e-310, 2.0 ** -1022, 1e-300, 1e-9, np.nextafter(1.0, 0.0),
             1.0 - 2.0 ** -52, 0.5, np.nextafter(0.5, 1.0), 0.3, 0.999]
    return [float(d) for d in spam + edges]


DTZ = [0.01, 0.3, np.nextafter(1.0, 0.0), 1e-300, 1e-320, float(np.nextafter(0.0, 1.0))]


def check(x, d, dtz, what):
    for k in KS:
        a, b = stepwise(x, d, dtz, k), chain(x, d, dtz, k)
        if not same_bits(a, b):
            i = int(np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0][0])
            raise AssertionError(f"{what}: d={d!r} dtz={dtz!r} k={k}: x={x[i]!r} stepwise {a[i]!r} chain {b[i]!r}")


@pytest.mark.parametrize("d", decays())
def test_random_values(d):
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(0, 1500, 4000), rng.uniform(0, 1, 2000), 10.0 ** rng.uniform(-330, 308, 4000),
                        -(10.0 ** rng.uniform(-330, 308, 1000))])
    for dtz in DTZ:
        check(x, d, dtz, "random")


@pytest.mark.parametrize("d", decays())
def test_values_crossing_the_threshold_at_every_step(d):
    """dtz / d**j, a few ulps either side: the value that reaches DecayToZero after
    exactly j of the k multiplies (j = 0: at the threshold as stored)."""
    for dtz in DTZ:
        xs = []
        with np.errstate(all="ignore"):
            for j in range(17):
                c = np.float64(dtz) / np.float64(d) ** j
                if not np.isfinite(c) or c <= 0:
                    continue
                xs += [ulps(c, n) for n in ULPS if c.view(np.int64) + n > 0]
                # (and the same reached by j exact-looking divisions, another rounding)
                c2 = np.float64(dtz)
                for _ in range(j):
                    c2 = c2 / np.float64(d)
                if np.isfinite(c2):
                    xs += [ulps(c2, n) for n in ULPS]
        x = np.array([v for v in xs if np.isfinite(v)], dtype=np.float64)
        assert len(x) > 0
        check(x, d, dtz, "crossing")


@pytest.mark.parametrize("d", decays())
def test_special_values(d):
    nan_pos = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    nan_neg = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]
    x = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -1022, 1e308, -1e308, np.finfo(np.float64).max,
                  np.inf, -np.inf, nan_pos, nan_neg, -1.0, -1e-3, -1500.0, 1.0, 0.01, 2.0 ** 63], dtype=np.float64)
    for dtz in DTZ:
        check(x, d, dtz, "special")


def test_no_decay_leaves_a_stored_value_under_the_threshold():
    x = np.array([0.001, -0.0, -5.0, 5e-324], dtype=np.float64)
    assert same_bits(chain(x, 0.5, 0.01, 0), x)
    assert same_bits(stepwise(x, 0.5, 0.01, 0), x)


def test_one_decay_is_decay():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 2, 1000)
    with np.errstate(all="ignore"):
        y = x * np.float64(0.9)
        want = np.where(y < 0.5, 0.0, y)
    assert same_bits(chain(x, 0.9, 0.5, 1), want)


@pytest.mark.parametrize("x,d,dtz,k", [
    (0.001, 3.0, 0.01, 3),      # d > 1: climbs back over the threshold
    (1.0, -0.5, 0.01, 2),       # d < 0: the sign alternates
    (-1e-320, 0.5, 0.0, 12),    # dtz == 0: -0.0 passes the one test
])
def test_outside_the_preconditions_the_forms_differ(x, d, dtz, k):
    """Why a decay the host did not validate (its weight is zero) and a DecayToZero of 0
    (no peer parameters set) keep the stepwise form on the device."""
    a, b = stepwise([x], d, dtz, k), chain([x], d, dtz, k)
    assert not same_bits(a, b)
