"""The zero map of the penalty counters (per 64-pair tile, topic and
counter MFP / IMD, "every present pair holds +0.0", which lets the refresh pass
skip the counter's load).  Every case starts from a state whose MFP and IMD are
zero everywhere (the map says zero for every tile), lets ONE operation store a
non-zero counter, refreshes twice, and then requires scores and exported state
bit-equal to the oracle and no map entry saying zero over a non-zero counter: a
writer that forgot its mark shows as a wrong score.

Overlay: about 200 nodes, d = 3: ~1.2k pairs in ~19 tiles, the last one partial.
T = 1 / 8 take the unrolled kernels, T = 3 the generic one."""
import numpy as np
import pytest

import gossip_cases as gc
import gsx
import oracle as orc
import propagation_cases as pc
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = pc.T0
N, D = 200, 3
TOPICS = [1, 3, 8]
THRESHOLDS = dict(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300, accept_px_threshold=0,
                  opportunistic_graft_threshold=5)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check(eng, ora, now, where=""):
    """Two refreshes, then the three assertions every case ends with."""
    for k in (1, 2):
        eng.refresh(now + k * S)
        ora.refresh(now + k * S)
    got, want = eng.scores(), ora.scores()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        f"{where}: scores differ at pairs {np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:8]}"
    gs, ws = eng.export_state(), ora.export_state()
    for f in abi.STATE_FIELDS:
        assert np.array_equal(bits(gs[f]), bits(ws[f])), f"{where}: state field {f}"
    assert eng.zero_map_violations() == 0, where
    return gs


def base_state(ov, T):
    """cfg3-style counters with MFP = IMD = 0; in-mesh records are active (grafted
    long ago), so about a quarter of them are under the P3 threshold."""
    st = synth.synthetic_state(ov, T, T0)
    st["mesh_failure_penalty"] = np.zeros_like(st["mesh_failure_penalty"])
    st["invalid_message_deliveries"] = np.zeros_like(st["invalid_message_deliveries"])
    in_mesh = (st["rec_flags"] & abi.GSX_REC_IN_MESH) != 0
    st["rec_flags"] = np.where(in_mesh, abi.GSX_REC_IN_MESH | abi.GSX_REC_ACTIVE, 0).astype(np.uint8)
    return st


def backends(T, st_edit=None, tp_edit=None, app=None):
    ov = synth.connect_some_overlay(N, d=D)
    assert ov.n_pairs % 64 != 0 and ov.n_pairs > 64 * 8
    st = base_state(ov, T)
    if st_edit:
        st_edit(ov, st)
    bes = []
    for be in (gsx.Engine(T), orc.Oracle(T)):
        be.set_peer_params(synth.bench_peer_params())
        for t in range(T):
            tp = synth.spam_test_topic_params()
            if tp_edit:
                tp_edit(tp)
            be.set_topic_params(t, tp)
        be.set_thresholds(abi.Thresholds(**THRESHOLDS))
        be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        be.import_state(st)
        be.set_app_scores(np.zeros(ov.n_pairs) if app is None else app(ov, st))
        bes.append(be)
    assert bes[0].zero_map_violations() == 0
    # the map says zero everywhere, but for the entries of what st_edit stored
    assert bes[0].zero_map_marked() == np.count_nonzero(tile_entries(st, T))
    return ov, st, bes[0], bes[1]


def tile_entries(st, T):
    """[tile][topic][counter]: some pair of the tile holds a non-zero MFP / IMD."""
    E = len(st["pair_flags"])
    nt = (E + 63) // 64
    out = np.zeros((nt, T, 2), dtype=bool)
    for k, f in enumerate(("mesh_failure_penalty", "invalid_message_deliveries")):
        nz = np.zeros((T, nt * 64), dtype=bool)
        nz[:, :E] = st[f].view(np.uint64).reshape(T, E) != 0
        out[:, :, k] = nz.reshape(T, nt, 64).any(axis=2).T
    return out


def events(bes, ev):
    for be in bes:
        be.apply_events(np.array(ev, dtype=abi.event_dtype()))


def under_threshold_record(ov, st, T):
    """(pair, topic) of an in-mesh active record with mmd under the P3 threshold,
    not in the first tile."""
    E = ov.n_pairs
    mmd = st["mesh_message_deliveries"].reshape(T, E)
    fl = st["rec_flags"].reshape(T, E)
    ok = ((fl & abi.GSX_REC_ACTIVE) != 0) & (mmd < 100.0)
    ok[:, :64] = False
    t, p = np.argwhere(ok)[0]
    return int(p), int(t)


def rec(st, T, field, p, t):
    return st[field].reshape(T, -1)[t, p]


@pytest.mark.parametrize("T", TOPICS)
def test_invalid_delivery_event(gpu_ok, T):
    ov, st, eng, ora = backends(T)
    p, t = 70, T - 1
    events((eng, ora), [(abi.EV_INVALID_DELIVERY, t, p, T0, 0)])
    assert eng.zero_map_marked() == 1
    out = check(eng, ora, T0, "EV_INVALID")
    assert eng.zero_map_marked() == 1
    assert rec(out, T, "invalid_message_deliveries", p, t) > 0


@pytest.mark.parametrize("T", TOPICS)
def test_prune_event_under_threshold(gpu_ok, T):
    ov, st, eng, ora = backends(T)
    p, t = under_threshold_record(ov, st, T)
    events((eng, ora), [(abi.EV_PRUNE, t, p, T0, 0)])
    assert eng.zero_map_marked() == 1
    out = check(eng, ora, T0, "EV_PRUNE")
    assert rec(out, T, "mesh_failure_penalty", p, t) > 0


@pytest.mark.parametrize("T", TOPICS)
def test_remove_peer_event_non_positive_score(gpu_ok, T):
    sel = {}

    def app(ov, st):
        sel["pt"] = under_threshold_record(ov, st, T)
        a = np.zeros(ov.n_pairs)
        a[sel["pt"][0]] = -1000.0  # score <= 0: RemovePeer retains the record and applies the mesh penalty
        return a

    ov, st, eng, ora = backends(T, app=app)
    p, t = sel["pt"]
    events((eng, ora), [(abi.EV_REMOVE_PEER, 0, p, T0, 0)])
    assert 1 <= eng.zero_map_marked() <= T  # one pair: at most one entry per topic
    out = check(eng, ora, T0, "EV_REMOVE_PEER")
    assert out["pair_flags"][p] == abi.GSX_PAIR_PRESENT
    assert rec(out, T, "mesh_failure_penalty", p, t) > 0


@pytest.mark.parametrize("T", TOPICS)
@pytest.mark.parametrize("mode", ["per-hop", "late", "user-deferred"])
def test_propagation_reject_credit(gpu_ok, T, mode):
    """Gossipsub batches holding ONE REJECT message each, from a state without any
    IMD, through every fold that credits P4 (gsx_engine.cpp prop_end):
    per-hop: hop latency 10 ms against pc.setup's 25 ms P3 window, so duplicates
      are counted per hop and the credits fold in k_prop_count, re-scoring as
      test_credit_threshold_crossings_between_calls does: at T = 1 its fused
      fold, at T > 1 fold_pair;
    late: no hop latency (every duplicate inside the window) and no first-deliverer
      rows: the deferred-fold call, whose P4 pairs fold at once in k_prop_defer;
    user-deferred: GSX_CREDIT_DEFER, folded by gsx_prop_fold_credits (k_prop_fold).
    Two consecutive calls, so the second starts from the forwarding state and the
    scores the first one's fold left."""
    ov = pc.overlay(N, D, seed=17)
    eng, ora = gsx.Engine(T), orc.Oracle(T)
    if mode == "late":
        eng.set_prop_tracking(False)
    for be in (eng, ora):
        pc.setup(be, ov, T, seed=17)  # AddPeer + Graft only: every MFP / IMD is zero
    assert eng.zero_map_marked() == 0
    lat = 0 if mode == "late" else 10
    for k in range(2):
        ms = pc.messages(N, 24, seed=17 + k)
        ms["validation"][5 + k] = abi.GSX_VALIDATION_REJECT
        cfg = pc.config(abi.GSX_ROUTER_GOSSIPSUB, topic=T - 1, latency_ms=lat, seed=9 + k)
        cfg.now_ns = T0 + (3 + k) * S
        want = ora.propagate(ms, cfg)[0].as_dict()
        if mode == "user-deferred":
            cfg.credit_scores = abi.GSX_CREDIT_DEFER
            eng.prop_begin(ms, cfg)
            for _ in range(cfg.max_hops):
                eng.prop_step(0)
            got = eng.prop_end().as_dict()
            eng.fold_credits()
        else:
            got = eng.propagate(ms, cfg)[0].as_dict()
        assert got == want and got["rejected"] > 0, k
        assert eng.zero_map_marked() > 0 and eng.zero_map_violations() == 0
        assert np.array_equal(eng.scores().view(np.uint64), ora.scores().view(np.uint64)), k
    out = check(eng, ora, T0 + 5 * S, "propagate REJECT, " + mode)
    imd_entries = np.count_nonzero(tile_entries(out, T)[:, :, 1])
    assert imd_entries > 0 and eng.zero_map_marked() == imd_entries  # (no MFP in this case)


@pytest.mark.parametrize("T", TOPICS)
def test_gossip_exchange_rejected_delivery(gpu_ok, T):
    """Heartbeat rounds with the gossip exchange on.  The batches between them run
    with credits off (GSX_CREDIT_OFF: propagation folds nothing, so no IMD comes
    from it) and hold invalid messages; those recovered by IWANT are the P4
    credits of the gossip fold (gx_credit), the only writer of IMD in this case."""
    bes = (gsx.Engine(T), orc.Oracle(T))
    res = [gc.exchange_run(be, T=T, ticks=6, invalid=0.3, credit=abi.GSX_CREDIT_OFF) for be in bes]
    assert res[0][1] == res[1][1]
    assert sum(o["gossip_rejected"] for o in res[0][1]) > 0
    out = check(*bes, T0 + 10 * S, "gossip exchange")
    assert np.count_nonzero(out["invalid_message_deliveries"]) > 0
    imd_entries = np.count_nonzero(tile_entries(out, T)[:, :, 1])
    assert imd_entries > 0 and bes[0].zero_map_marked() >= imd_entries


@pytest.mark.parametrize("T", TOPICS)
def test_heartbeat_prunes_under_delivering_peer(gpu_ok, T):
    """A heartbeat prunes a negative-score mesh peer whose active record is under
    the P3 threshold: the mesh failure penalty of the heartbeat's own prune."""
    sel = {}

    def app(ov, st):
        sel["pt"] = under_threshold_record(ov, st, T)
        a = np.zeros(ov.n_pairs)
        a[sel["pt"][0]] = -1000.0
        return a

    ov, st, eng, ora = backends(T, app=app)
    p, t = sel["pt"]
    for be in (eng, ora):
        be.refresh(T0 + S)  # (scores the heartbeat reads)
    assert eng.zero_map_violations() == 0
    go = eng.heartbeat(1, T0 + 2 * S, 5).as_dict()
    wo = ora.heartbeat(1, T0 + 2 * S, 5).as_dict()
    assert go == wo and go["prunes"] > 0
    out = check(eng, ora, T0 + 2 * S, "heartbeat prune")
    assert rec(out, T, "mesh_failure_penalty", p, t) > 0


@pytest.mark.parametrize("T", TOPICS)
def test_import_single_non_zero(gpu_ok, T):
    def edit(ov, st):
        st["invalid_message_deliveries"][(T - 1) * ov.n_pairs + 130] = 3.0

    ov, st, eng, ora = backends(T, st_edit=edit)
    assert eng.zero_map_marked() == 1
    out = check(eng, ora, T0, "import")
    assert rec(out, T, "invalid_message_deliveries", 130, T - 1) > 0


@pytest.mark.parametrize("T", TOPICS)
def test_synthesize_with_sybils(gpu_ok, T):
    """Device-synthesized state whose sybils (the upper half of the nodes) hold
    invalid-message counters; the oracle starts from the engine's export."""
    ov, st, eng, ora = backends(T)
    eng.synthesize_state(abi.SynthSpec(seed=3, now_ns=T0, fmd_max=1500.0, mmd_max=400.0, mfp_max=0.0,
                                       imd_max_sybil=100.0, p_in_mesh=0.5, graft_window_ns=2 * abi.HOUR, bp_max=5.0,
                                       p_disconnected=0.05, p_absent=0.05, expire_jitter_ns=4 * S,
                                       sybil_first_node=N // 2))
    assert eng.zero_map_violations() == 0
    st = eng.export_state()
    # no MFP (mfp_max = 0); the marks are those of the tiles holding a sybil's IMD and no others
    present = np.tile(st["pair_flags"] != 0, T)
    assert np.count_nonzero(st["invalid_message_deliveries"][~present]) == 0
    assert eng.zero_map_marked() == np.count_nonzero(tile_entries(st, T))
    ora.import_state(st)
    out = check(eng, ora, T0, "synthesize")
    imd = out["invalid_message_deliveries"].reshape(T, -1)
    assert np.count_nonzero(imd) > 0 and np.count_nonzero(imd[:, ov.col < N // 2]) == 0


@pytest.mark.parametrize("T", TOPICS)
def test_purge_then_add_peer(gpu_ok, T):
    """A retained pair holding a non-zero IMD expires (purged by a refresh), then
    the peer is added again: its records are zero again, the mark may stay."""
    p = 200

    def edit(ov, st):
        st["invalid_message_deliveries"][p] = 7.0
        st["pair_flags"][p] = abi.GSX_PAIR_PRESENT  # retained
        st["expire_ns"][p] = T0 + S // 2

    ov, st, eng, ora = backends(T, st_edit=edit)
    for be in (eng, ora):
        be.refresh(T0 + S)
    assert eng.export_state()["pair_flags"][p] == 0
    events((eng, ora), [(abi.EV_ADD_PEER, 0, p, T0 + S, 0)])
    assert eng.zero_map_marked() == 1  # an absent lane in the tile: the mark stays
    out = check(eng, ora, T0 + S, "purge, AddPeer")
    assert out["pair_flags"][p] != 0 and rec(out, T, "invalid_message_deliveries", p, 0) == 0
    assert eng.zero_map_marked() == 0  # all 64 pairs present and zero again: cleared


@pytest.mark.parametrize("T", TOPICS)
def test_decay_to_zero_clears_and_remarks(gpu_ok, T):
    """IMD decays by 0.5 per refresh to under DecayToZero = 0.01 (1 -> 0 in 7
    refreshes): the tile's mark is cleared, and a later invalid delivery on the
    same tile is seen again."""
    def tp_edit(tp):
        tp.invalid_message_deliveries_decay = 0.5

    ov, st, eng, ora = backends(T, tp_edit=tp_edit)
    p, t = 64 * 3 + 5, T - 1
    events((eng, ora), [(abi.EV_INVALID_DELIVERY, t, p, T0, 0)])
    now = T0
    for k in range(9):
        now += S
        eng.refresh(now)
        ora.refresh(now)
        assert eng.zero_map_violations() == 0
        # 0.5 ** 6 = 0.0156 is kept, 0.5 ** 7 = 0.0078 < 0.01 becomes 0: the 7th refresh clears the mark
        assert eng.zero_map_marked() == (1 if k < 6 else 0), k
    out = check(eng, ora, now, "decayed")
    assert rec(out, T, "invalid_message_deliveries", p, t) == 0
    assert eng.zero_map_marked() == 0
    events((eng, ora), [(abi.EV_INVALID_DELIVERY, t, p + 9, now + 2 * S, 0)])
    assert eng.zero_map_marked() == 1
    out = check(eng, ora, now + 2 * S, "re-marked")
    assert rec(out, T, "invalid_message_deliveries", p + 9, t) > 0
