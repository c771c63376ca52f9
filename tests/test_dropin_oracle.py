"""The drivers of dropin_cases.py on the oracle alone (CPU): the preconditions that make
test_gpu_dropin.py's comparisons meaningful, pinned so that a change of seed or shape cannot
hollow them out."""
import numpy as np
import pytest

import dropin_cases as dc
import oracle as orc
from dropin_cases import HUB, MAX_EVENTS, MAX_OBS, MAX_PAIRS
from gsx import abi
from pair_epoch_cases import CONNECTED, RETAINED


def changed(a, b):
    return a.view(np.uint64) != b.view(np.uint64)


@pytest.fixture(scope="module")
def mixed_run():
    return dc.run_mixed(dc.Lockstep(orc.Oracle(3)), 3)


def test_mixed_overlay_shape():
    ov = dc.mixed()
    hub = ov.row_ptr[HUB + 1] - ov.row_ptr[HUB]
    assert 9000 < ov.n_pairs <= MAX_PAIRS and ov.n_pairs % 64 and ov.n % 64
    assert hub >= 1100 and hub > dc.BLOCK and hub < 2 * dc.BLOCK  # the stride loop runs twice
    ips = ov.node_ips[ov.col[ov.row_ptr[HUB]:ov.row_ptr[HUB + 1]]][:, 0]
    assert np.bincount(ips).max() >= 20  # many colocated peers in the hub's row


def test_batches_sit_on_the_limits(mixed_run):
    by = {b.name: b for b, _, _, _ in mixed_run}
    for n in (2, 63, 64, 65):
        b = by[f"{n} observers"]
        assert len(b.observers) == n and b.expect == (1 if n <= MAX_OBS else 0)
        if n > 2:
            # row groups and pairs-only groups, interleaved in the issue order
            assert 0 < len(b.rows) < n
            obs = dc.mixed().pair_observer()
            order = [int(obs[e[2]]) for e in b.events]
            assert order != sorted(order) and len(b.near) == 16 and len(b.far) == 16
    for n in (MAX_EVENTS, MAX_EVENTS + 1):
        b = by[f"{n} events"]
        assert len(b.events) == n and b.observers == [HUB] and b.rows == [HUB]
        assert b.expect == (1 if n == MAX_EVENTS else 0)
    assert all(b.expect == 1 for b in by.values() if b.name not in ("65 observers", f"{MAX_EVENTS + 1} events"))
    assert not by["pairs only, one event"].rows and not by["pairs only, five observers"].rows
    assert len(by["pairs only, five observers"].observers) == 5
    first = by["every kind in the hub's row"]
    assert sorted({e[0] for e in first.events}) == list(range(1, 10)) and first.observers == [HUB]
    assert len(first.pairs) == 10  # each kind on a pair of its own (the RemovePeers with their EV_APP_SCORE)
    one = by["300 events on one pair"]
    assert len(one.events) == 300 and len(one.pairs) == 1
    assert [e[0] for e in one.events].index(abi.EV_PRUNE) == 149
    dup = by["duplicate pairs"]
    apps = [e for e in dup.events if e[0] == abi.EV_APP_SCORE and e[2] == dup.events[0][2]]
    assert len(apps) == 2 and apps[0][4] != apps[1][4]
    for b in by.values():
        assert not set(b.unnamed) & set(b.pairs)


def test_every_batch_changes_scores_and_the_hub_row_moves_unnamed_pairs(mixed_run):
    ov = dc.mixed()
    obs = ov.pair_observer()
    for b, before, after, st in mixed_run:
        ch = changed(before, after)
        assert ch[b.pairs].any(), b.name
        assert not ch[b.far].any(), b.name  # untouched rows keep their scores
    by = {b.name: (b, x, y, st) for b, x, y, st in mixed_run}
    b, before, after, _ = by["hub row only"]
    assert b.rows == [HUB] and len(b.observers) == 11
    unnamed = np.ones(ov.n_pairs, dtype=bool)
    unnamed[b.pairs] = False
    assert (changed(before, after) & unnamed & (obs == HUB)).sum() >= 20
    assert changed(before, after)[b.near].any()
    # a retained and a forgotten RemovePeer
    b, _, _, st = by["every kind in the hub's row"]
    removed = [e[2] for e in b.events if e[0] == abi.EV_REMOVE_PEER]
    assert [int(st["pair_flags"][p]) for p in removed] == [RETAINED, 0]
    # 300 events: the deliveries ran into their caps
    b, _, _, st = by["300 events on one pair"]
    p, T, E = b.pairs[0], 3, ov.n_pairs
    t = p % T
    _, tps = dc.rz.scenario_params(T)
    assert st["first_message_deliveries"][t * E + p] == tps[t].first_message_deliveries_cap
    assert st["invalid_message_deliveries"][t * E + p] > 80


@pytest.mark.parametrize("E", [MAX_PAIRS, MAX_PAIRS + 1])
def test_exact_overlays(E):
    ov, before, after = dc.run_exact(dc.Lockstep(orc.Oracle(1)), E)
    assert ov.n_pairs == E == len(ov.col) == ov.row_ptr[-1] and ov.n == dc.EXACT_N
    assert ov.row_ptr[0] == 0 and (np.diff(ov.row_ptr) >= 8).all()
    obs = ov.pair_observer()
    assert (ov.col != obs).all() and ((0 <= ov.col) & (ov.col < ov.n)).all()
    for u in (0, 1, 4000, ov.n - 1):
        row = ov.col[ov.row_ptr[u]:ov.row_ptr[u + 1]]
        assert (np.diff(row) > 0).all()
    key = set(zip(obs.tolist(), ov.col.tolist()))
    one_way = [(u, v) for u, v in key if (v, u) not in key]
    assert one_way == ([] if E == MAX_PAIRS else [(0, 100)])
    ch = changed(before, after)
    assert ch[5] and ch[8 * 4000 + 2] and ch.sum() >= 3  # the RemovePeer moved a neighbour's P6


@pytest.mark.parametrize("T", [1, 3, 9])
def test_pending_decays_cross_decay_to_zero(T):
    rec = bp = 0
    for phase in (5, 12):
        r, b, flags = dc.run_pending_decays(dc.Lockstep(orc.Oracle(T)), T, phase)
        assert flags == (RETAINED, 0)
        rec, bp = rec + r, bp + b
    assert rec > 0 and bp > 0


@pytest.mark.parametrize("name", list(dc.MUTATORS))
def test_mutator_changes_the_oracle_scores(name):
    ls = dc.Lockstep(orc.Oracle(dc.C_T))
    before, after, c = dc.run_mutator(ls, name)
    must = dc.MUTATORS[name][2]
    if len(before) == len(after):
        assert changed(before, after).any() == must, name
    else:
        assert must and name.startswith("load_overlay")
    if name.startswith("heartbeat"):
        h = c.hb_totals
        assert h["prunes"] > 0 and h["grafts"] > 0 and h["iwant_served"] > 0 and h["broken_promises"] > 0, h


def test_shortcut_pairs_move_as_claimed():
    out = dc.run_shortcut(dc.Lockstep(orc.Oracle(3)))
    assert out["other row"][0] == out["other row"][1]
    for step in ("the pair", "AddPeer in the row", "RemovePeer in the row"):
        assert out[step][0] != out[step][1], step


@pytest.mark.parametrize("T", [1, 3, 9])
def test_session_holds_every_kind_of_call(T):
    ops, reads = dc.run_session(dc.Lockstep(orc.Oracle(T)), T, 1)
    kinds = {op[0] for op in ops}
    assert {"events", "trace", "refresh", "propagate", "heartbeat", "score", "score_many", "scores", "check"} <= kinds
    big = [op[1] for op in ops[3:] if op[0] == "events" and len(op[1]) > 100]
    assert big and len(reads) > 100
