"""The drop-in Score() path against the oracle: gsx_score / gsx_score_many on an engine of at
most 65,536 pairs answer from a host copy of the scores, skip the device when no queued
event touches the pair, and otherwise apply the queued events and re-score what they change
in one k_dropin launch (gsx_engine.cpp dropin_fast).  Every other GPU test reads scores
through scores() / export_state(), which never use that copy.

The drivers are dropin_cases.py's (test_dropin_oracle.py pins their preconditions on the
CPU).  Every read is compared with the oracle's bit for bit (view(np.uint64) for scores,
view(np.uint8) for every field of abi.STATE_FIELDS), and dropin_launches() says which path
answered: every k_dropin limit (64 / 65 observers, 4,096 / 4,097 events, 65,536 / 65,537
pairs), both block sizes, a row longer than the block, mixed row / pair groups and events
under 5 and 12 pending decays assert the launch they claim."""
import numpy as np
import pytest

import dropin_cases as dc
import gsx
import oracle as orc
import pair_epoch_cases as pe

pytestmark = pytest.mark.gpu


def lockstep(T):
    return dc.Lockstep(gsx.Engine(T), orc.Oracle(T))


def test_batch_shapes_and_limits_through_one_launch(gpu_ok):
    """(a) on mixed(): every event kind in the hub's row (1,100 pairs: the 1,024-thread block
    strides twice), 2 / 63 / 64 observers with row and pairs-only groups interleaved (65: the
    general path), the hub as the only row re-scored, 300 events on one pair, duplicates,
    pairs-only batches (the 256-thread launch), 4,096 events (4,097: the general path)."""
    ls = lockstep(3)
    out = dc.run_mixed(ls, 3)
    want = {b.name: b.expect for b, _, _, _ in out}
    assert ls.eng.dropin_launches() == sum(want.values()) == len(want) - 2
    assert [e for _, e in ls.counted] == list(want.values())


@pytest.mark.parametrize("E", [dc.MAX_PAIRS, dc.MAX_PAIRS + 1])
def test_pair_limit(gpu_ok, E):
    """65,536 pairs: the host copy and k_dropin; 65,537: the gather path, no launch."""
    ls = lockstep(1)
    dc.run_exact(ls, E)
    assert ls.eng.dropin_launches() == (1 if E == dc.MAX_PAIRS else 0)


@pytest.mark.parametrize("T", [1, 3, 9])
def test_events_with_decays_pending(gpu_ok, T):
    """(b) every event kind, a retaining and a forgetting RemovePeer, through k_dropin with 5
    and with 12 decays pending (test_gpu_wb16.start's state), then four more refreshes; a
    touched counter and a penalty cross DecayToZero while 5 or more decays pend."""
    rec = bp = 0
    for phase in (5, 12):
        ls = lockstep(T)
        r, b, flags = dc.run_pending_decays(ls, T, phase, check=lambda where: pe.same(ls.eng, ls.ora, where))
        assert flags == (pe.RETAINED, 0) and ls.eng.dropin_launches() == 1
        rec, bp = rec + r, bp + b
    assert rec > 0 and bp > 0


@pytest.mark.parametrize("name", list(dc.MUTATORS))
def test_no_mutator_leaves_a_stale_host_copy(gpu_ok, name):
    """(c) prime the host copy, run the mutator, then score(p) of 64 pairs one by one,
    score_many(all pairs), scores() and export_state(), then one event of each kind read
    through score_many: all equal to the oracle.  The oracle has no write-back period and keeps
    no first-deliverer rows, so set_decay_writeback and set_prop_tracking run on the engine
    alone (neither changes a result); it credits a propagation at once, so the engine's
    GSX_CREDIT_DEFER + fold is compared with the oracle's GSX_CREDIT_NOW."""
    ls = lockstep(dc.C_T)
    before, after, _ = dc.run_mutator(ls, name)
    if len(before) == len(after):
        assert (before.view(np.uint64) != after.view(np.uint64)).any() == dc.MUTATORS[name][2]


def test_shortcut_skips_the_device_only_when_it_may(gpu_ok):
    """(d) a queued event on p does not launch for a read of another row's q, does for p; a
    queued AddPeer / RemovePeer launches for another pair of its row (whose P6 moved); an
    out-of-range pair is GSX_ERANGE and leaves the queued events queued."""
    ls = lockstep(3)
    out = dc.run_shortcut(ls)
    assert out["other row"][0] == out["other row"][1]
    for step in ("the pair", "AddPeer in the row", "RemovePeer in the row"):
        assert out[step][0] != out[step][1], step
    assert ls.eng.dropin_launches() == 4


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("T", [1, 3, 9])
def test_seeded_router_session(gpu_ok, T, seed):
    """(e) randomized.session_ops: make_ops plus large event batches, credited gossipsub /
    floodsub batches, heartbeats, score, score_many and scores() in between."""
    ls = lockstep(T)
    _, reads = dc.run_session(ls, T, seed)
    assert len(reads) > 100
