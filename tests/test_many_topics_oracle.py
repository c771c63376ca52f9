"""The CPU oracle above 8 topics.  tests/test_gpu_many_topics.py trusts the
oracle at topic counts up to 64, where the reference's known answers
(tests/golden/) never go, so the oracle is pinned here by relabelling: for
code with no per-topic randomness, a run in which only topic k of 64 is
scored, meshed and used must equal the one-topic run on topic 0.  The
heartbeat's draws are keyed by the topic, so for it the checks are that no
exported word carries a topic >= T and that a ninth, weightless topic leaves
the other eight as an eight-topic run has them.

The scenarios of the GPU file are run here on the oracle alone as well: what
each of them must reach (a topic >= 8, bit 32, bit 63, counters non-zero)
holds for the oracle's own results, before any engine is compared with it."""
import numpy as np
import pytest

import gossip_cases as gc
import heartbeat_cases as hc
import many_topics_cases as M
import oracle as orc
import propagation_cases as pc
import randomized as R
from gsx import abi

S = abi.SECOND


# ---- relabelling ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scoring_world():
    ov = R.small_overlay(300, 3, 5, 50)
    ops = R.make_ops(ov, 1, 5, n_steps=300)
    want = M.one_topic_replay(orc.Oracle(1), ov, 1, 0, ops)
    assert M.counters_seen(want)
    assert any(op[0] == "topic_params" for op in ops) and any(op[0] == "gc" for op in ops)
    return ov, ops, want


@pytest.mark.parametrize("k", M.RELABEL_TOPICS)
def test_scoring_on_topic_k_of_64_equals_the_one_topic_run(scoring_world, k):
    ov, ops, want = scoring_world
    got = M.one_topic_replay(orc.Oracle(64), ov, 64, k, ops)
    M.assert_relabelled(got, want, 64, k, ov.n_pairs)


@pytest.mark.parametrize("router", [abi.GSX_ROUTER_GOSSIPSUB, abi.GSX_ROUTER_FLOODSUB], ids=["gossipsub", "floodsub"])
def test_credited_propagation_on_topic_k_of_64_equals_the_one_topic_run(router):
    want = M.prop_relabel_run(orc.Oracle(1), 1, 0, router)
    for k in M.RELABEL_TOPICS:
        M.assert_prop_relabelled(M.prop_relabel_run(orc.Oracle(64), 64, k, router), want, k)


# ---- heartbeat -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [9, 33])
def test_no_exported_word_carries_a_topic_beyond_T(T):
    """joined and fanout are 64-bit words whatever T is: after joins, leaves, fanout
    publishes and expiries on the highest topics no bit >= T is set; the backoff
    and IHAVE arrays have T rows and hold entries in the last one."""
    ov, outs, snaps, mems, _ = M.member_run(orc.Oracle(T), T)
    beyond = ~np.uint64((1 << T) - 1)
    for joined, fanout, lastpub in mems:
        assert not (joined & beyond).any() and not (fanout & beyond).any()
        assert lastpub.shape == (ov.n, T)
    assert any(M.bit(m[0], T - 1).any() for m in mems) and any(M.bit(m[1], T - 1).any() for m in mems)
    for s in snaps:
        assert s["backoff"].shape == (T, ov.n_pairs)
    assert any(s["backoff"][T - 1].any() for s in snaps)


def _eight_of(be, T, ticks=4):
    """pc.setup's mesh on T topics; topics >= 8 weigh nothing in the score; traffic on topics 0..7."""
    n, seed = 260, 300
    ov = pc.overlay(n, 6, seed, mix_protocols=True, direct_frac=0.03)
    pc.setup(be, ov, T, seed, mesh_degree=2)
    for t in range(8, T):
        be.set_topic_params(t, hc._zero_weight_topic())
    rng = np.random.default_rng(seed + 2)  # (pc.setup's own app scores are drawn after its T meshes)
    be.set_app_scores(np.where(rng.random(ov.n_pairs) < 0.08, -500.0, np.abs(rng.normal(0, 2, ov.n_pairs))))
    be.refresh(pc.T0 + 2 * S + S // 2)
    flags, outs = [], []
    for k in range(ticks):
        now = pc.T0 + (3 + k) * S
        outs.append(be.heartbeat(58 + k, now, 77).as_dict())
        flags.append(be.export_state()["rec_flags"].reshape(T, ov.n_pairs)[:8].copy())
        cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=k % 8, latency_ms=5, seed=seed + k)
        cfg.now_ns = now + 100 * abi.MILLISECOND
        be.propagate(pc.messages(n, 48, seed + 1000 * k), cfg)
        be.refresh(now + 500 * abi.MILLISECOND)
    return flags, outs


def test_a_ninth_weightless_topic_leaves_the_first_eight_alone():
    """The heartbeat's draws depend on (node, tick, topic), not on T: with a ninth
    topic that contributes nothing to the scores, topics 0..7 are grafted and
    pruned exactly as in the eight-topic run, round by round."""
    f8, o8 = _eight_of(orc.Oracle(8), 8)
    f9, o9 = _eight_of(orc.Oracle(9), 9)
    assert sum(o["grafts"] for o in o8) > 0 and sum(o["prunes"] for o in o8) > 0
    assert sum(o["grafts"] for o in o9) > sum(o["grafts"] for o in o8)  # (topic 8 ran too)
    for k, (a, b) in enumerate(zip(f8, f9)):
        assert np.array_equal(a, b), (k, np.argwhere(a != b)[:5].tolist())


# ---- what the GPU file's scenarios reach, on the oracle alone ------------------------------
@pytest.mark.parametrize("case", M.HB_CASES, ids=M.hb_id)
def test_heartbeat_cases_reach_the_high_topics(case):
    M.hb_reach(case, *M.hb_run(orc.Oracle(case[0]), case))


def test_hub_case_reaches_topic_8():
    ov, n = M.hub_overlay()
    M.hub_reach(ov, 9, *M.hub_run(orc.Oracle(9), ov, n))


@pytest.mark.parametrize("T", [33, 64])
def test_membership_cases_reach_bits_32_and_63(T):
    ov, outs, _, mems, _ = M.member_run(orc.Oracle(T), T)
    M.member_reach(T, ov, outs, mems)
    M.px_member_reach(T, M.px_member_run(orc.Oracle(T), T))


@pytest.mark.parametrize("T", sorted(M.GX_CASES))
def test_exchange_cases_reach_the_last_topic(T):
    _, outs, snaps, _ = gc.exchange_run(orc.Oracle(T), **M.GX_CASES[T])
    M.gx_reach(T, outs, snaps)


@pytest.mark.parametrize("topic", [8, 32])
def test_credit_case_reaches_its_topic(topic):
    ora = orc.Oracle(M.CREDIT_T)
    ov = M.credit_world(ora)
    for i, (m, ms) in enumerate(M.credit_batches(ov.n)):
        now = pc.T0 + (3 + i) * S
        before = ora.export_state()
        out = ora.propagate(ms, M.credit_config(topic, abi.GSX_CREDIT_NOW, now))[0].as_dict()
        M.credit_reach(M.CREDIT_T, topic, ov.n_pairs, ms, out, before, ora.export_state())
        ora.refresh(now + S // 2)


def test_sharded_case_has_cross_shard_control_on_topic_32():
    ora = orc.Oracle(M.SHARD_T)
    ov, _ = M.shard_world(ora)
    flags = M.shard_rounds(ora, ov)[1]
    M.shard_reach(ov, flags)
