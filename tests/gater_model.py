"""A plain restatement of the reference's peer gater (peer_gater.go) and of
GossipSubRouter.AcceptFrom's last stage, one call at a time on a simulated
clock.  Dicts keyed as the Go maps are (peerStats by peer, ipStats by IP
string), Python floats (binary64), and the canonical draw in place of
rand.Float64().  It is the checker of the engine's gater: nothing here knows
about groups ids, integer counts or kernels.
"""
from __future__ import annotations

ACCEPT_NONE, ACCEPT_CONTROL, ACCEPT_ALL = 0, 1, 2
M64 = (1 << 64) - 1
NEVER = None  # the zero time.Time of lastThrottle

REJECT_QUEUE_FULL = "validation queue full"
REJECT_THROTTLED = "validation throttled"
REJECT_IGNORED = "validation ignored"
REJECT_FAILED = "validation failed"


def smix(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def h4(seed: int, tag: int, a: int, b: int) -> int:
    """The engine's counter hash (SplitMix64 finalisers), gsx.h."""
    return smix((seed + 0x9E3779B97F4A7C15 * (1 + smix(tag ^ smix(a ^ smix(b))))) & M64)


def canonical_u(seed: int, pair: int, draw: int) -> float:
    """u = (h4(seed, 14, pair, draw) >> 11) * 2^-53: Go's Int63n(1 << 53) / 2^53 shape."""
    return (h4(seed, 14, pair, draw) >> 11) * 2.0 ** -53


class Params:
    """PeerGaterParams, peer_gater.go:31-55 (durations in ns)."""

    def __init__(self, threshold, global_decay, source_decay, decay_interval=10 ** 9, decay_to_zero=0.01,
                 retain_stats=6 * 3600 * 10 ** 9, quiet=60 * 10 ** 9, duplicate_weight=0.125, ignore_weight=1.0,
                 reject_weight=16.0, topic_delivery_weights=None):
        # NewPeerGaterParams, :98-111
        self.threshold = threshold
        self.global_decay = global_decay
        self.source_decay = source_decay
        self.decay_interval = decay_interval
        self.decay_to_zero = decay_to_zero
        self.retain_stats = retain_stats
        self.quiet = quiet
        self.duplicate_weight = duplicate_weight
        self.ignore_weight = ignore_weight
        self.reject_weight = reject_weight
        self.topic_delivery_weights = dict(topic_delivery_weights or {})

    def validate(self):
        """:57-88 -> an error string or None"""
        if self.threshold <= 0:
            return "invalid Threshold"
        if self.global_decay <= 0 or self.global_decay >= 1:
            return "invalid GlobalDecay"
        if self.source_decay <= 0 or self.source_decay >= 1:
            return "invalid SourceDecay"
        if self.decay_interval < 10 ** 9:
            return "invalid DecayInterval"
        if self.decay_to_zero <= 0 or self.decay_to_zero >= 1:
            return "invalid DecayToZero"
        if self.quiet < 10 ** 9:
            return "invalid Quiet"
        if self.duplicate_weight <= 0:
            return "invalid DuplicateWeight"
        if self.ignore_weight < 1:
            return "invalid IgnoreWeight"
        if self.reject_weight < 1:
            return "invalid RejectWeight"
        return None


class Stats:
    """peerGaterStats, :143-151"""

    def __init__(self):
        self.connected = 0
        self.expire = 0  # the zero time: before every `now`
        self.deliver = self.duplicate = self.ignore = self.reject = 0.0


class PeerGater:
    """peerGater, :119-141.  get_ip(peer) -> the IP string ("<unknown>" for none), :280-317."""

    def __init__(self, params: Params, get_ip):
        self.params = params
        self.validate = 0.0
        self.throttle = 0.0
        self.last_throttle = NEVER
        self.peer_stats = {}
        self.ip_stats = {}
        self.get_ip = get_ip

    # :219-259
    def decay_stats(self, now: int):
        p = self.params
        self.validate *= p.global_decay
        if self.validate < p.decay_to_zero:
            self.validate = 0.0
        self.throttle *= p.global_decay
        if self.throttle < p.decay_to_zero:
            self.throttle = 0.0
        for ip in list(self.ip_stats):
            st = self.ip_stats[ip]
            if st.connected > 0:
                for f in ("deliver", "duplicate", "ignore", "reject"):
                    v = getattr(st, f) * p.source_decay
                    setattr(st, f, 0.0 if v < p.decay_to_zero else v)
            elif st.expire < now:
                del self.ip_stats[ip]

    # :261-278
    def get_peer_stats(self, peer) -> Stats:
        st = self.peer_stats.get(peer)
        if st is None:
            ip = self.get_ip(peer)
            st = self.ip_stats.get(ip)
            if st is None:
                st = self.ip_stats[ip] = Stats()
            self.peer_stats[peer] = st
        return st

    # :320-363; u: the draw standing in for rand.Float64()
    def accept_from(self, peer, now: int, u: float) -> int:
        p = self.params
        if self.last_throttle is NEVER or now - self.last_throttle > p.quiet:
            return ACCEPT_ALL
        if self.throttle == 0:
            return ACCEPT_ALL
        if self.validate != 0 and self.throttle / self.validate < p.threshold:
            return ACCEPT_ALL
        st = self.get_peer_stats(peer)
        total = st.deliver + p.duplicate_weight * st.duplicate + p.ignore_weight * st.ignore + p.reject_weight * st.reject
        if total == 0:
            return ACCEPT_ALL
        threshold = (1 + st.deliver) / (1 + total)
        if u < threshold:
            return ACCEPT_ALL
        return ACCEPT_CONTROL

    # :369-386
    def add_peer(self, peer):
        self.get_peer_stats(peer).connected += 1

    def remove_peer(self, peer, now: int):
        st = self.get_peer_stats(peer)
        st.connected -= 1
        st.expire = now + self.params.retain_stats
        del self.peer_stats[peer]

    # :393-443
    def validate_message(self):
        self.validate += 1

    def deliver_message(self, peer, topic):
        st = self.get_peer_stats(peer)
        weight = self.params.topic_delivery_weights.get(topic, 0.0)
        if weight == 0:
            weight = 1.0
        st.deliver += weight

    def reject_message(self, peer, reason: str, now: int):
        if reason in (REJECT_QUEUE_FULL, REJECT_THROTTLED):
            self.last_throttle = now
            self.throttle += 1
        elif reason == REJECT_IGNORED:
            self.get_peer_stats(peer).ignore += 1
        else:
            self.get_peer_stats(peer).reject += 1

    def duplicate_message(self, peer):
        self.get_peer_stats(peer).duplicate += 1
