"""Shared helpers of test_gpu_purge_skip.py and test_gpu_bp_deferred.py: a small
overlay (197 pairs: three full tiles of 64 and a partial one, rows of about six
pairs so that many span a tile boundary, six nodes to an IP), backends loaded
with one state, and a bit-for-bit comparison of engine and oracle."""
import numpy as np

import gsx
import nonfinite_cases as nc
import oracle as orc
from gsx import abi, synth

S = abi.SECOND
T0 = nc.T0
E = nc.E
CONNECTED = abi.GSX_PAIR_PRESENT | abi.GSX_PAIR_CONNECTED
RETAINED = abi.GSX_PAIR_PRESENT
THRESHOLDS = dict(gossip_threshold=-100, publish_threshold=-200, graylist_threshold=-300, accept_px_threshold=0,
                  opportunistic_graft_threshold=5)


def f64_bits(x):
    return int(np.float64(x).view(np.int64))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(eng, ora, where):
    """Scores and every exported state array bit-identical; the exported pair flags carry
    nothing but PRESENT | CONNECTED.  -> the engine's export."""
    got, want = eng.scores(), ora.scores()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), \
        f"{where}: scores differ at pairs {np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:8]}"
    gs, ws = eng.export_state(), ora.export_state()
    for f in abi.STATE_FIELDS:
        assert np.array_equal(bits(gs[f]), bits(ws[f])), \
            f"{where}: state field {f} at {np.nonzero(np.asarray(gs[f]) != np.asarray(ws[f]))[0][:8]}"
    assert gs["last_refresh_ns"] == ws["last_refresh_ns"], where
    assert (gs["pair_flags"] & ~np.uint8(CONNECTED)).max() == 0, where
    assert eng.zero_map_violations() == 0 and eng.pair_zero_map_violations() == 0, where
    return gs


def peer_params(retain_ns=3 * S, d7=0.5, dtz=0.3, thr6=1):
    pp = synth.bench_peer_params()
    pp.retain_score_ns = retain_ns
    pp.behaviour_penalty_decay = d7
    pp.decay_to_zero = dtz
    pp.ip_colocation_factor_threshold = thr6
    return pp


def configure(be, T, ov, pp):
    be.set_peer_params(pp)
    for t in range(T):
        be.set_topic_params(t, synth.spam_test_topic_params())
    be.set_thresholds(abi.Thresholds(**THRESHOLDS))
    be.load_overlay(ov.row_ptr, ov.col, ov.edge_flags, ov.node_ips)


def backends(T, pp=None, st=None, ov=None, extra=0):
    """-> (overlay, [engines..., oracle]) loaded with `st` (default: every pair but a tenth
    connected, none retained) and zero app scores."""
    ov = ov or nc.overlay()
    if st is None:
        st = synth.synthetic_state(ov, T, T0, p_absent=0.1)
    bes = [gsx.Engine(T) for _ in range(1 + extra)] + [orc.Oracle(T)]
    for be in bes:
        configure(be, T, ov, pp or peer_params())
        be.import_state(st)
        be.set_app_scores(np.zeros(ov.n_pairs))
    return ov, bes


def events(bes, ev):
    for be in bes:
        be.apply_events(np.array(ev, dtype=abi.event_dtype()))


def remove_events(p, now, score):
    """RemovePeer of pair p at `now` after its app score is set to `score` (<= 0: the peer is
    retained; > 0: forgotten, score.go:615)."""
    return [(abi.EV_APP_SCORE, 0, int(p), now, f64_bits(score)), (abi.EV_REMOVE_PEER, 0, int(p), now, 0)]


class Clock:
    def __init__(self, *bes, now=T0):
        self.bes, self.now, self.n = bes, now, 0

    def at(self, now, where):
        """One refresh of every backend at `now`; engine == oracle after it."""
        assert now > self.now
        self.now = now
        for be in self.bes:
            be.refresh(now)
        self.n += 1
        return same(self.bes[0], self.bes[-1], f"{where}: refresh #{self.n} at T0 + {now - T0} ns")

    def step(self, where, k=1, dt=S):
        for _ in range(k):
            out = self.at(self.now + dt, where)
        return out
