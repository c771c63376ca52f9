"""traffic_model.py against the CPU oracle: the model's class rows per pair are the rows
the oracle's first deliverers and duplicate rows give, its totals the oracle's gsx_prop_out
scalars (graylisted included), and the vectorised reduction from class rows to the five
tables is the brute-force loop's.  No device work here (CPU suite)."""
import numpy as np
import pytest

import traffic_cases as tc
import traffic_model as tm

KEYS = [k for k in tc.CASES if tc.model_applies(k)]


@pytest.mark.parametrize("key", KEYS)
def test_model_rows_are_the_oracles(key):
    x = tc.reference(key)
    ov, ms, cfg, _ = tc.inputs(key)
    m, R = len(ms), x.model
    got = {c: tm.bits_of_ints(R.rows[c], m) for c in range(tm.COLS)}
    assert np.array_equal(got[tm.FIRST] | got[tm.INVALID], x.B[tm.FIRST] | x.B[tm.INVALID])
    assert np.array_equal(got[tm.FIRST], x.B[tm.FIRST]) and np.array_equal(got[tm.INVALID], x.B[tm.INVALID])
    assert np.array_equal(got[tm.DUP], x.B[tm.DUP])
    assert np.array_equal(got[tm.SENT], x.B[tm.SENT])
    o = x.out
    assert (R.transmissions, R.deliveries, R.duplicates, R.invalid, R.graylisted) == \
        (o["transmissions"], o["deliveries"], o["duplicates"], o["rejected"] + o["ignored"], o["graylisted"])


def test_the_cases_reach_every_class():
    tot = np.zeros(tm.COLS, dtype=np.int64)
    for key in KEYS:
        tot += tc.reference(key).B.sum((1, 2), dtype=np.int64)
    assert (tot > 0).all(), tot
    assert tc.reference("invalid").B[tm.INVALID].any() and tc.reference("gossip-m300").B[tm.GRAYLISTED].any()
    assert tc.reference("cut1").out["hops"] == 1 and tc.reference("cut2").out["hops"] == 2


@pytest.mark.parametrize("kind", ["null", "planes"])
def test_vectorised_tables_equal_the_loop(kind):
    x = tc.reference("gossip-m65")
    ov, ms, _, _ = tc.inputs("gossip-m65")
    sz = tc.sizes(kind, len(ms))
    for a, b in zip(tm.tables(x.B, ov.row_ptr, ov.col, sz), tm.tables_loop(x.B, ov.row_ptr, ov.col, sz)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    msg, node, nbytes, pair, pbytes = tm.tables(x.B, ov.row_ptr, ov.col, sz)
    assert msg[:, tm.SENT].sum() == x.out["transmissions"] == pair.sum() == node[:, tm.SENT].sum()
    assert nbytes[:, 0].sum() == nbytes[:, 1].sum() == pbytes.sum()
