"""gsx_refresh launches the purge of expired retained peers only while a retained
pair (present, not connected) can exist: after a RemovePeer, an imported state
that holds one or a synthesized state with p_disconnected > 0, until a refresh
later than every such pair's expiry.  A missing launch would leave an expired
pair present and the IP colocation counts of its group too high, so every
refresh compares scores and the whole exported state with the oracle bit for
bit, and purge_launches() says which refreshes launched.

Shapes: 197 pairs (three full tiles and a partial one, rows spanning the tile
boundaries), T = 1 and T = 8; RetainScore 3 s."""
import numpy as np
import pytest

import gsx
import pair_epoch_cases as pe
from gsx import abi
from pair_epoch_cases import CONNECTED, RETAINED, S, T0

pytestmark = pytest.mark.gpu

RETAIN = 3 * S


def connected(st, k, skip=()):
    """k connected pairs of an exported state, spread over the tiles."""
    c = [int(p) for p in np.nonzero(st["pair_flags"] == CONNECTED)[0] if int(p) not in skip]
    assert len(c) >= 4 * k
    return c[:: len(c) // k][:k]


@pytest.mark.parametrize("T", [1, 8])
def test_purge_launched_only_while_a_pair_can_be_retained(gpu_ok, T):
    ov, (eng, ora) = pe.backends(T, pe.peer_params(retain_ns=RETAIN))
    # a synthesized state without disconnected pairs, handed to the oracle through an export
    eng.synthesize_state(abi.SynthSpec(seed=11, now_ns=T0, fmd_max=1500.0, mmd_max=400.0, mfp_max=50.0,
                                       imd_max_sybil=100.0, p_in_mesh=0.5, graft_window_ns=2 * abi.HOUR, bp_max=5.0,
                                       p_disconnected=0.0, p_absent=0.1, expire_jitter_ns=4 * S,
                                       sybil_first_node=ov.n))
    ora.import_state(eng.export_state())
    ck = pe.Clock(eng, ora)
    st = ck.step("synthesized, none disconnected", 3)
    assert eng.purge_launches() == 0 and (st["pair_flags"] == RETAINED).sum() == 0

    # RemovePeer: score <= 0 retains, score > 0 forgets; both at `now`
    used = set()
    neg, pos = connected(st, 4), connected(st, 4, skip=connected(st, 4))
    used.update(neg + pos)
    t = ck.now
    pe.events((eng, ora), sum((pe.remove_events(p, t, -1e6) for p in neg), []) +
              sum((pe.remove_events(p, t, 1e6) for p in pos), []))
    st = pe.same(eng, ora, "RemovePeer")
    assert (st["pair_flags"][neg] == RETAINED).all() and (st["pair_flags"][pos] == 0).all()
    assert (st["expire_ns"][neg] == t + RETAIN).all() and eng.purge_launches() == 0
    st = ck.at(t + S, "before the expiry")
    assert eng.purge_launches() == 1 and (st["pair_flags"][neg] == RETAINED).all()
    st = ck.at(t + RETAIN, "at the expiry (purged only after it)")
    assert eng.purge_launches() == 2 and (st["pair_flags"][neg] == RETAINED).all()
    st = ck.at(t + RETAIN + 1, "one ns after the expiry")
    assert eng.purge_launches() == 3 and (st["pair_flags"][neg] == 0).all()
    ck.step("nothing retained any more", 3)
    assert eng.purge_launches() == 3

    # a retained pair reconnects before its expiry: the horizon stands until it has passed
    (p,) = connected(st, 1, skip=used)
    used.add(p)
    t = ck.now
    pe.events((eng, ora), pe.remove_events(p, t, -1e6))
    ck.at(t + S, "retained")
    pe.events((eng, ora), [(abi.EV_ADD_PEER, 0, p, ck.now, 0)])
    st = pe.same(eng, ora, "reconnected")
    assert st["pair_flags"][p] == CONNECTED and eng.purge_launches() == 4
    st = ck.at(t + RETAIN + 1, "past the reconnected pair's old expiry")
    assert st["pair_flags"][p] == CONNECTED and eng.purge_launches() == 5
    ck.step("reconnected, nothing retained", 2)
    assert eng.purge_launches() == 5

    # a second RemovePeer after the flag had cleared
    t = ck.now
    pe.events((eng, ora), pe.remove_events(p, t, -1e6))
    st = ck.at(t + S, "retained again")
    assert st["pair_flags"][p] == RETAINED and eng.purge_launches() == 6
    st = ck.at(t + RETAIN + 1, "expired again")
    assert st["pair_flags"][p] == 0 and eng.purge_launches() == 7
    ck.step("cleared again", 2)
    assert eng.purge_launches() == 7

    # two RemovePeers with different `now`, the later one queued first: the later horizon governs
    a, b = connected(st, 2, skip=used)
    used.update((a, b))
    t = ck.now
    pe.events((eng, ora), pe.remove_events(b, t + 2 * S, -1e6) + pe.remove_events(a, t, -1e6))
    st = ck.at(t + RETAIN + 1, "the earlier one expired")
    assert st["pair_flags"][a] == 0 and st["pair_flags"][b] == RETAINED and eng.purge_launches() == 8
    st = ck.at(t + 2 * S + RETAIN, "the later one at its expiry")
    assert st["pair_flags"][b] == RETAINED and eng.purge_launches() == 9
    st = ck.at(t + 2 * S + RETAIN + 1, "the later one expired")
    assert st["pair_flags"][b] == 0 and eng.purge_launches() == 10
    ck.step("both gone", 2)
    assert eng.purge_launches() == 10

    # import_state with retained pairs in it (expiries 1 s and 2 s ahead), then one without
    ret = connected(st, 6, skip=used)
    imp = {f: (v.copy() if isinstance(v, np.ndarray) else v) for f, v in ora.export_state().items()}
    imp["pair_flags"][ret] = RETAINED
    imp["expire_ns"][ret] = ck.now + S * (1 + np.arange(len(ret)) % 2)
    for f in ("rec_flags", "mesh_time_ns"):  # RemovePeer took them out of every mesh
        imp[f].reshape(T, -1)[:, ret] = 0
    for be in (eng, ora):
        be.import_state(imp)
    t = ck.now
    pe.same(eng, ora, "imported with retained pairs")
    st = ck.at(t + S + 1, "half of the imported retained pairs expired")
    assert eng.purge_launches() == 11
    assert sorted(st["pair_flags"][ret].tolist()) == [0] * 3 + [RETAINED] * 3
    st = ck.at(t + 2 * S + 1, "all of them expired")
    assert eng.purge_launches() == 12 and (st["pair_flags"][ret] == 0).all()
    ck.step("none left", 2)
    for be in (eng, ora):
        be.import_state(ora.export_state())
    ck.step("imported without retained pairs", 2)
    assert eng.purge_launches() == 12

    # synthesize_state with p_disconnected > 0: expiries within 2 s either side of its `now`
    # (no record in a mesh: RemovePeer leaves a retained pair in none)
    t = ck.now + S
    eng.synthesize_state(abi.SynthSpec(seed=12, now_ns=t, fmd_max=1500.0, mmd_max=400.0, mfp_max=50.0,
                                       imd_max_sybil=100.0, p_in_mesh=0.0, graft_window_ns=2 * abi.HOUR, bp_max=5.0,
                                       p_disconnected=0.25, p_absent=0.1, expire_jitter_ns=4 * S,
                                       sybil_first_node=ov.n))
    st = eng.export_state()
    n_ret = int((st["pair_flags"] == RETAINED).sum())
    assert n_ret > 20 and st["expire_ns"][st["pair_flags"] == RETAINED].max() <= t + 2 * S
    ora.import_state(st)
    ck.now = t
    st = ck.at(t + 1, "synthesized: the expiries before its now")
    left = int((st["pair_flags"] == RETAINED).sum())
    assert 0 < left < n_ret and eng.purge_launches() == 13
    st = ck.at(t + 2 * S + 2, "synthesized: past every expiry")
    assert (st["pair_flags"] == RETAINED).sum() == 0 and eng.purge_launches() == 14
    ck.step("synthesized: none left", 3)
    assert eng.purge_launches() == 14

    # a new overlay restarts the count
    eng.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
    assert eng.purge_launches() == 0


@pytest.mark.parametrize("T", [1, 8])
def test_expiry_moves_the_ip_colocation_of_the_group(gpu_ok, T):
    """Three pairs of one observer share an IP, one above IPColocationFactorThreshold = 2; one of
    them is retained and expires: the P6 of the two others drops to zero at exactly that refresh
    (their group's count is the purge's), on the engine as on the oracle."""
    ov = pe.nc.overlay()
    # a row with a pair either side of a tile boundary B: the retained pair is the last of its tile
    B, u = next((b, i) for b in (64, 128, 192) for i in range(ov.n)
                if ov.row_ptr[i] <= b - 2 and b + 1 <= ov.row_ptr[i + 1] - 1)
    trio = [B - 1, B, B + 1]
    assert all(ov.row_ptr[u] <= p < ov.row_ptr[u + 1] for p in trio)
    ov.node_ips[:, 0] = 1000 + np.arange(ov.n)  # every node its own IP, but the trio's peers
    ov.node_ips[ov.col[trio], 0] = 7
    st = pe.synth.synthetic_state(ov, T, T0)
    ov, (eng, ora) = pe.backends(T, pe.peer_params(retain_ns=RETAIN, thr6=2), st=st, ov=ov)
    ck = pe.Clock(eng, ora)
    ck.step("start", 2)
    assert eng.purge_launches() == 0
    others = trio[1:]
    for be in (eng, ora):
        assert (be.snapshot()["ip_colocation_factor"][trio] == 1.0).all()
    t = ck.now
    pe.events((eng, ora), pe.remove_events(trio[0], t, -1e6))
    ck.at(t + S, "retained: still counted")
    ck.at(t + RETAIN, "at the expiry: still counted")
    for be in (eng, ora):
        assert (be.snapshot()["ip_colocation_factor"][trio] == 1.0).all()
    st = ck.at(t + RETAIN + 1, "expired: the group is down to two")
    assert st["pair_flags"][trio[0]] == 0 and eng.purge_launches() == 3
    for be in (eng, ora):
        assert (be.snapshot()["ip_colocation_factor"][others] == 0.0).all()
    ck.step("after", 2)
    assert eng.purge_launches() == 3
