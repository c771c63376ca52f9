"""The pair zero map (per 64-pair tile one entry for the
application scores and one for the IP colocation factors, "every one is +0.0",
which lets the refresh pass skip app[p], ipg[p] and the ipcount gathers).  After
every call: scores and exported state bit-equal to the oracle, no entry of the
pair map and none of the zero map saying zero over a non-zero value.  A writer
that forgot its mark shows as a wrong score at the next refresh.

Overlay: a hub (node 0) with 70 peers, each of which also has two ring
neighbours: 280 pairs, four whole tiles and a tail tile of 24.  The hub's row is
pairs 0 .. 69: it crosses the tile boundary at 64, and hub pair k is the pair
with node k + 1.  Pairs 66 and 272 start absent, 100 and 150 retained; tiles 0,
2 and 3 are all present, so a refresh can clear them, tiles 1 and 4 cannot.
T = 1 / 8 take the unrolled kernels, T = 3 the generic one."""
import numpy as np
import pytest

import gsx
import nonfinite_cases as nc
import oracle as orc
import randomized as R
from gsx import abi, synth

pytestmark = pytest.mark.gpu

S = abi.SECOND
T0 = R.T0
TOPICS = [1, 3, 8]
HUB_DEG = 70
E = HUB_DEG * 4
ABSENT, RETAINED = (66, 272), (100, 150)
APP, P6 = abi.GSX_PZ_APP, abi.GSX_PZ_P6
FAR = 10_000  # IPs no node starts with


def overlay(shared=()):
    """shared: (node a, node b) pairs, b gets a's IP."""
    n = HUB_DEG + 1
    rows = [list(range(1, n))]
    for i in range(1, n):
        rows.append(sorted({0, (i - 2) % HUB_DEG + 1, i % HUB_DEG + 1}))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    col = np.concatenate(rows).astype(np.int32)
    ips = np.full((n, 2), abi.GSX_NO_IP, dtype=np.uint32)
    ips[:, 0] = np.arange(n, dtype=np.uint32)
    for a, b in shared:
        ips[b, 0] = ips[a, 0]
    ov = synth.Overlay(n, row_ptr, col, np.full(len(col), abi.GSX_EDGE_GOSSIPSUB, dtype=np.uint8), ips,
                       np.zeros(n, dtype=bool))
    assert ov.n_pairs == E and row_ptr[1] == HUB_DEG > 64
    return ov


def state(ov, T):
    st = synth.synthetic_state(ov, T, T0)
    st["pair_flags"][list(ABSENT)] = 0
    st["pair_flags"][list(RETAINED)] = abi.GSX_PAIR_PRESENT
    for p in RETAINED:  # as RemovePeer leaves them: outside every mesh
        st["rec_flags"].reshape(T, E)[:, p] = 0
        st["mesh_time_ns"].reshape(T, E)[:, p] = 0
    st["expire_ns"][:] = T0 + 1000 * S
    return st


def peer_params(**kw):
    pp = synth.bench_peer_params()  # AppSpecificWeight 1, P6 weight -10, threshold 1
    for k, v in kw.items():
        setattr(pp, k, v)
    return pp


def backends(T, shared=(), pp=None, st_edit=None):
    ov = overlay(shared)
    st = state(ov, T)
    if st_edit:
        st_edit(st)
    eng, ora = gsx.Engine(T), orc.Oracle(T)
    for be in (eng, ora):
        be.set_peer_params(pp or peer_params())
        for t in range(T):
            be.set_topic_params(t, synth.spam_test_topic_params())
        be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)
        be.import_state(st)
    # a fresh map says nothing
    assert eng.pair_zero_map_marked(APP) == eng.pair_zero_map_marked(P6) == (E + 63) // 64
    same(eng, ora, "loaded")
    return ov, st, eng, ora


def same(eng, ora, where):
    nc.assert_same(eng.scores(), ora.scores(), f"{where}: scores")
    gs, ws = eng.export_state(), ora.export_state()
    for f in abi.STATE_FIELDS:
        nc.assert_same(gs[f], ws[f], f"{where}: state field {f}")
    assert gs["last_refresh_ns"] == ws["last_refresh_ns"], where
    assert eng.pair_zero_map_violations() == 0, where
    assert eng.zero_map_violations() == 0, where
    return ws


class Clock:
    def __init__(self, eng, ora):
        self.bes, self.now, self.n = (eng, ora), T0, 0

    def refresh(self, where, k=1):
        for _ in range(k):
            self.now += S
            self.n += 1
            for be in self.bes:
                be.refresh(self.now)
            ws = same(*self.bes, f"{where}: refresh {self.n}")
        return ws


def call(bes, name, *a):
    for be in bes:
        getattr(be, name)(*a)
    same(*bes, name)


def events(bes, ev):
    call(bes, "apply_events", np.array(ev, dtype=abi.event_dtype()))


def app_event(p, v, now=T0):
    return (abi.EV_APP_SCORE, 0, p, now, int(np.float64(v).view(np.int64)))


def cannot_clear(pair_flags):
    """Tiles with an absent pair, and the tail tile."""
    pf = np.zeros((E + 63) // 64 * 64, dtype=bool)
    pf[:E] = (np.asarray(pair_flags) & abi.GSX_PAIR_PRESENT) != 0
    return ~pf.reshape(-1, 64).all(axis=1)


def p6_tiles(ora):
    """Tiles holding a present pair with a non-zero IP colocation factor (the oracle's)."""
    f = np.zeros((E + 63) // 64 * 64)
    f[:E] = ora.snapshot()["ip_colocation_factor"]
    return f.reshape(-1, 64).any(axis=1)


def p6_of(ora, p):
    return float(ora.snapshot()["ip_colocation_factor"][p])


def make_positive(st, T, p):
    """Pair p scores above zero (first deliveries only): a RemovePeer forgets it."""
    for f in ("mesh_failure_penalty", "invalid_message_deliveries", "mesh_message_deliveries"):
        st[f].reshape(T, E)[:, p] = 0.0
    st["rec_flags"].reshape(T, E)[:, p] = 0
    st["mesh_time_ns"].reshape(T, E)[:, p] = 0
    st["behaviour_penalty"][p] = 0.0


# ---- application scores -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", TOPICS)
def test_app_zero_event_and_back(gpu_ok, T):
    ov, st, eng, ora = backends(T)
    bes = (eng, ora)
    ck = Clock(eng, ora)
    call(bes, "set_app_scores", np.zeros(E))
    ws = ck.refresh("all zero")
    stuck = int(cannot_clear(ws["pair_flags"]).sum())
    assert stuck == 2 and eng.pair_zero_map_marked(APP) == stuck  # tiles 1 (pair 66 absent) and 4 (the tail)
    p = 64 * 2 + 9  # tile 2 says zero
    before = ora.scores()[p]
    events(bes, [app_event(p, -7.5, ck.now)])  # (same() reads the scores: the masked pass sees it at once)
    assert ora.scores()[p] < before - 7.4 and eng.pair_zero_map_marked(APP) == stuck + 1
    ck.refresh("one app score")
    assert eng.snapshot()["app_specific_score"][p] == -7.5 and eng.pair_zero_map_marked(APP) == stuck + 1
    events(bes, [app_event(p, 0.0, ck.now)])
    assert eng.pair_zero_map_marked(APP) == stuck + 1  # a store of +0.0 clears nothing: only a refresh does
    ck.refresh("back to zero")
    assert eng.pair_zero_map_marked(APP) == stuck
    ck.refresh("a whole write-back cycle", 4)
    assert eng.pair_zero_map_marked(APP) == stuck


@pytest.mark.parametrize("T", TOPICS)
def test_app_bulk_set_with_negative_zero(gpu_ok, T):
    ov, st, eng, ora = backends(T)
    bes = (eng, ora)
    ck = Clock(eng, ora)
    call(bes, "set_app_scores", np.zeros(E))
    ck.refresh("all zero")
    assert eng.pair_zero_map_marked(APP) == 2
    app = np.zeros(E)
    app[5] = -0.0  # not +0.0: tile 0 is marked (and -0.0 * 1 + score == score either way)
    app[64 * 3 + 1] = 2.25
    app[RETAINED[0]] = -1.0  # tile 1, marked already
    call(bes, "set_app_scores", app)
    assert eng.pair_zero_map_marked(APP) == 4
    ck.refresh("bulk", 2)
    assert eng.pair_zero_map_marked(APP) == 4
    call(bes, "set_app_scores", np.zeros(E))
    assert eng.pair_zero_map_marked(APP) == 4
    ck.refresh("zero again")
    assert eng.pair_zero_map_marked(APP) == 2


@pytest.mark.parametrize("T", TOPICS)
def test_app_infinity_times_zero_weight(gpu_ok, T):
    """+inf * 0 is a NaN the skipped load would lose: the product is executed from the loaded value."""
    ov, st, eng, ora = backends(T, pp=peer_params(app_specific_weight=0.0))
    bes = (eng, ora)
    ck = Clock(eng, ora)
    call(bes, "set_app_scores", np.zeros(E))
    ck.refresh("all zero")
    p = 64 * 3 + 17
    events(bes, [app_event(p, np.inf, ck.now)])
    ck.refresh("inf", 2)
    assert np.isnan(ora.scores()[p]) and np.isnan(eng.scores()[p])
    assert np.count_nonzero(np.isnan(ora.scores())) == 1


@pytest.mark.parametrize("T", TOPICS)
def test_app_event_between_masked_score_passes(gpu_ok, T):
    """scores() after events re-scores only the marked rows (the masked pass, which reads PZ_APP)."""
    ov, st, eng, ora = backends(T)
    bes = (eng, ora)
    ck = Clock(eng, ora)
    call(bes, "set_app_scores", np.zeros(E))
    ck.refresh("all zero")
    p = 64 * 2 + 30
    events(bes, [(abi.EV_PENALTY, 0, p + 1, ck.now, 2)])  # (same() reads the scores: one masked pass)
    before = ora.scores()[p]
    events(bes, [app_event(p, 3.0, ck.now)])
    assert ora.scores()[p] > before + 2.9
    events(bes, [(abi.EV_PENALTY, 0, p, ck.now, 1)])
    ck.refresh("after")


# ---- IP colocation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TOPICS)
def test_p6_unique_ips(gpu_ok, T):
    ov, st, eng, ora = backends(T)
    ck = Clock(eng, ora)
    ws = ck.refresh("unique IPs")
    assert not p6_tiles(ora).any()
    assert eng.pair_zero_map_marked(P6) == int(cannot_clear(ws["pair_flags"]).sum()) == 2
    events((eng, ora), [(abi.EV_ADD_PEER, 0, ABSENT[0], ck.now, 0)])  # its own IP: at the threshold, no mark
    assert eng.pair_zero_map_marked(P6) == 2
    ck.refresh("AddPeer, own IP")
    assert eng.pair_zero_map_marked(P6) == 1  # tile 1 is whole now


@pytest.mark.parametrize("T", TOPICS)
def test_p6_add_peer_other_tile_remove_purge(gpu_ok, T):
    """Hub pair 66 (node 67, absent, tile 1) shares its IP with hub pair 2 (node 3, tile 0)."""
    ov, st, eng, ora = backends(T, shared=[(3, 67)])
    bes = (eng, ora)
    ck = Clock(eng, ora)
    ck.refresh("one present pair on the IP")
    assert not p6_tiles(ora).any() and eng.pair_zero_map_marked(P6) == 2  # tile 0 says zero
    events(bes, [(abi.EV_ADD_PEER, 0, 66, ck.now, 0)])
    assert eng.pair_zero_map_marked(P6) == 3  # both tiles of the hub's row, and the tail
    ck.refresh("two on the IP")
    assert p6_of(ora, 2) == p6_of(ora, 66) == 1.0 and ora.scores()[66] == -10.0
    assert list(np.nonzero(p6_tiles(ora))[0]) == [0, 1]
    assert eng.pair_zero_map_marked(P6) == 3
    # RemovePeer retains it (score <= 0), the retention runs out, the purge takes the count back
    events(bes, [(abi.EV_REMOVE_PEER, 0, 66, ck.now, 0)])
    ws = ck.refresh("retained")
    assert ws["pair_flags"][66] == abi.GSX_PAIR_PRESENT and eng.pair_zero_map_marked(P6) == 3
    ws = ck.refresh("purged", 11)
    assert ws["pair_flags"][66] == 0 and not p6_tiles(ora).any()
    assert eng.pair_zero_map_marked(P6) == 2  # tile 0 cleared; tile 1 has the absent pair again


@pytest.mark.parametrize("T", TOPICS)
def test_p6_add_peer_same_tile(gpu_ok, T):
    """Hub pair 10 leaves with a positive score (forgotten), learns the IP of hub pair 4 while
    absent, and comes back: both are in tile 0, which said zero."""
    ov, st, eng, ora = backends(T, st_edit=lambda st: make_positive(st, T, 10))
    bes = (eng, ora)
    ck = Clock(eng, ora)
    ck.refresh("unique IPs")
    assert eng.pair_zero_map_marked(P6) == 2 and ora.scores()[10] > 0
    events(bes, [(abi.EV_REMOVE_PEER, 0, 10, ck.now, 0)])
    assert ora.export_state()["pair_flags"][10] == 0
    call(bes, "set_pair_ips", np.array([10], dtype=np.uint64), np.array([[5, abi.GSX_NO_IP]], dtype=np.uint32))
    assert eng.pair_zero_map_marked(P6) == 2  # an absent pair only records the list
    events(bes, [(abi.EV_ADD_PEER, 0, 10, ck.now, 0)])
    assert eng.pair_zero_map_marked(P6) == 3
    ck.refresh("two on the IP")
    assert p6_of(ora, 4) == p6_of(ora, 10) == 1.0 and ora.scores()[10] == -10.0
    assert list(np.nonzero(p6_tiles(ora))[0]) == [0]


@pytest.mark.parametrize("T", TOPICS)
def test_p6_set_pair_ips_and_whitelist(gpu_ok, T):
    a, b, c = 154, 155, 156  # a ring node's row of three pairs, in tile 2
    ov, st, eng, ora = backends(T, st_edit=lambda st: make_positive(st, T, c))
    assert int(ov.row_ptr[29]) == a and int(ov.row_ptr[30]) == c + 1
    bes = (eng, ora)
    ck = Clock(eng, ora)
    ck.refresh("unique IPs")
    assert eng.pair_zero_map_marked(P6) == 2
    ips = np.array([[FAR, abi.GSX_NO_IP], [FAR, FAR + 1]], dtype=np.uint32)
    call(bes, "set_pair_ips", np.array([a, b], dtype=np.uint64), ips)
    assert eng.pair_zero_map_marked(P6) == 3
    ck.refresh("moved onto one IP")
    assert p6_of(ora, a) == p6_of(ora, b) == 1.0 and eng.pair_zero_map_marked(P6) == 3
    call(bes, "set_ip_whitelist", [FAR])  # no penalty any more; every entry marked, cleared by the refresh
    ck.refresh("whitelisted")
    assert not p6_tiles(ora).any() and eng.pair_zero_map_marked(P6) == 2
    # a third pair joins the whitelisted group by AddPeer: counted, never penalised, no mark needed
    events(bes, [(abi.EV_REMOVE_PEER, 0, c, ck.now, 0)])
    assert ora.export_state()["pair_flags"][c] == 0
    call(bes, "set_pair_ips", np.array([c], dtype=np.uint64), np.array([[FAR, abi.GSX_NO_IP]], dtype=np.uint32))
    events(bes, [(abi.EV_ADD_PEER, 0, c, ck.now, 0)])
    ck.refresh("three on a whitelisted IP", 2)
    assert not p6_tiles(ora).any()
    call(bes, "set_ip_whitelist", [])
    ck.refresh("whitelist dropped")
    assert p6_of(ora, c) == 4.0 and list(np.nonzero(p6_tiles(ora))[0]) == [2]


@pytest.mark.parametrize("T", TOPICS)
def test_p6_set_peer_params(gpu_ok, T):
    """Nodes 3, 4 and 5 (hub pairs 2, 3, 4) share one IP under threshold 3: no P6 until it is lowered
    (then also in node 4's own row, tile 1, which holds 3 and 5)."""
    ov, st, eng, ora = backends(T, shared=[(3, 4), (3, 5)], pp=peer_params(ip_colocation_factor_threshold=3))
    bes = (eng, ora)
    ck = Clock(eng, ora)
    ck.refresh("threshold 3")
    assert not p6_tiles(ora).any() and eng.pair_zero_map_marked(P6) == 2
    call(bes, "set_peer_params", peer_params(ip_colocation_factor_threshold=1))
    ck.refresh("threshold 1")
    assert p6_of(ora, 3) == 4.0  # (3 - 1) ** 2
    assert list(np.nonzero(p6_tiles(ora))[0]) == [0, 1] and eng.pair_zero_map_marked(P6) == 3
    call(bes, "set_peer_params", peer_params(ip_colocation_factor_weight=0.0))
    ck.refresh("w6 = 0", 2)
    call(bes, "set_peer_params", peer_params())
    ck.refresh("w6 back", 2)
    assert eng.pair_zero_map_marked(P6) == 3


@pytest.mark.parametrize("T", TOPICS)
def test_p6_import_state_with_colocation(gpu_ok, T):
    """Hub pair 66 is absent in the first state and present in the imported one."""
    ov, st, eng, ora = backends(T, shared=[(3, 67)])
    bes = (eng, ora)
    ck = Clock(eng, ora)
    ck.refresh("one present pair on the IP")
    assert eng.pair_zero_map_marked(P6) == 2
    st2 = dict(ora.export_state())
    st2["pair_flags"] = st2["pair_flags"].copy()
    st2["pair_flags"][66] = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
    call(bes, "import_state", st2)
    ck.refresh("imported")
    assert list(np.nonzero(p6_tiles(ora))[0]) == [0, 1] and p6_of(ora, 2) == p6_of(ora, 66) == 1.0
    assert eng.pair_zero_map_marked(P6) == 3


# ---- everything at once ---------------------------------------------------------------------------------
class Checked:
    """An engine whose every call is followed by the two maps' checks."""

    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        f = getattr(self._e, name)

        def g(*a, **kw):
            out = f(*a, **kw)
            if self._e.n_pairs:
                assert self._e.pair_zero_map_violations() == 0, name
                assert self._e.zero_map_violations() == 0, name
            return out

        return g if callable(f) else f


@pytest.mark.parametrize("T", [3, 8])
def test_random_calls_with_colocated_ips(gpu_ok, T):
    ov = R.small_overlay(90, 3, 5, 12)  # 12 IPs for 90 nodes: most groups are shared
    ops = R.make_ops(ov, T, 5, n_steps=150)
    eng = gsx.Engine(T)
    got = R.replay(Checked(eng), ov, T, ops)
    want = R.replay(orc.Oracle(T), ov, T, ops)
    assert len(got) == len(want) > 3
    for k, (g, w) in enumerate(zip(got, want)):
        nc.assert_same(g[0], w[0], f"check {k}: scores")
        for f in abi.STATE_FIELDS:
            nc.assert_same(g[1][f], w[1][f], f"check {k}: {f}")
        assert g[2] == w[2]
    assert eng.pair_zero_map_marked(P6) > 0


@pytest.mark.parametrize("T", TOPICS)
def test_engine_reuse_second_overlay(gpu_ok, T):
    """A larger and a smaller overlay loaded on the engine after the first: every map starts over."""
    ov, st, eng, ora = backends(T)
    ck = Clock(eng, ora)
    call((eng, ora), "set_app_scores", np.zeros(E))
    ck.refresh("first overlay")
    assert eng.pair_zero_map_marked(APP) == eng.pair_zero_map_marked(P6) == 2
    for n, d, seed in ((60, 3, 9), (20, 2, 4)):
        ov2 = R.small_overlay(n, d, seed, 6)
        E2 = ov2.n_pairs
        st2 = synth.synthetic_state(ov2, T, T0)
        app = np.zeros(E2)
        app[E2 // 2] = 1.5
        for be in (eng, ora):
            be.load_overlay(ov2.row_ptr, ov2.col, ov2.edge_flags, ov2.node_ips)
        assert eng.pair_zero_map_marked(APP) == eng.pair_zero_map_marked(P6) == (E2 + 63) // 64
        for be in (eng, ora):
            be.import_state(st2)
            be.set_app_scores(app)
        for k in (1, 2):
            for be in (eng, ora):
                be.refresh(T0 + k * S)
            same(eng, ora, f"overlay of {n}: refresh {k}")
        assert n < 60 or np.count_nonzero(ora.snapshot()["ip_colocation_factor"]) > 0
