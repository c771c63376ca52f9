"""A line-by-line Python model of tag_tracer.go over a minimal connection
manager: Protect / Unprotect, decaying tags with BumpSumBounded(0, cap) and
DecayFixed(amount), and the engine's forced-trim contract (gsx.h,
gsx_conn_trim).  One TagTracer is one observer's tracer; peers are any
hashable ids."""
from __future__ import annotations

REJECT_THROTTLED = "validation throttled"
REJECT_IGNORED = "validation ignored"
REJECT_FAILED = "validation failed"


class Params:
    def __init__(self, bump=1, decay_amount=1, cap=15, decay_interval_ns=600 * 10 ** 9):
        # GossipSubConnTagBumpMessageDelivery / DecayAmount / MessageDeliveryCap / DecayInterval, tag_tracer.go:13-31
        self.bump, self.decay_amount, self.cap, self.decay_interval_ns = bump, decay_amount, cap, decay_interval_ns


class DecayingTag:
    """connmgr.DecayingTag with BumpSumBounded(min, max) and DecayFixed(minuend)."""

    def __init__(self, mgr, name, lo, hi, minuend):
        self.mgr, self.name, self.lo, self.hi, self.minuend = mgr, name, lo, hi, minuend
        self.closed = False

    def bump(self, p, delta):
        if self.closed:
            raise RuntimeError("decaying tag closed")
        tags = self.mgr.tags.setdefault(p, {})
        v = tags.get(self.name, 0) + delta  # BumpSumBounded: the sum, clamped
        tags[self.name] = min(self.hi, max(self.lo, v))

    def decay(self):  # DecayFixed: (value - minuend, remove when the result is <= 0)
        for tags in self.mgr.tags.values():
            if self.name in tags:
                v = tags[self.name] - self.minuend
                if v <= 0:
                    del tags[self.name]
                else:
                    tags[self.name] = v

    def close(self):  # removes the tag from every peer
        self.closed = True
        for tags in self.mgr.tags.values():
            tags.pop(self.name, None)
        self.mgr.decaying.pop(self.name, None)


class ConnManager:
    def __init__(self):
        self.protected = {}  # peer -> set of tags
        self.tags = {}       # peer -> {tag name: value}
        self.decaying = {}

    def protect(self, p, tag):
        self.protected.setdefault(p, set()).add(tag)

    def unprotect(self, p, tag):
        s = self.protected.get(p)
        if s is None:
            return False
        s.discard(tag)
        if not s:
            del self.protected[p]
            return False
        return True

    def is_protected(self, p, tag=""):
        s = self.protected.get(p)
        if not s:
            return False
        return True if tag == "" else tag in s

    def register_decaying_tag(self, name, lo, hi, minuend):
        if name in self.decaying:
            raise RuntimeError("decaying tag already registered")
        t = DecayingTag(self, name, lo, hi, minuend)
        self.decaying[name] = t
        return t

    def tick(self, steps=1):
        """`steps` decay intervals of every registered tag."""
        for _ in range(steps):
            for t in list(self.decaying.values()):
                t.decay()

    def tag_value(self, p, name):
        return self.tags.get(p, {}).get(name, 0)

    def tag_exists(self, p, name):
        return name in self.tags.get(p, {})

    def value(self, p):  # GetTagInfo(p).Value
        return sum(self.tags.get(p, {}).values())

    def trim(self, conns, low_water):
        """The engine's forced TrimOpenConns: `conns` the open connections as peers
        in index order; -> the positions closed: the first min(len - low_water,
        unprotected) unprotected ones by ascending (value, position)."""
        if len(conns) <= low_water:
            return []
        cand = sorted((self.value(p), i) for i, p in enumerate(conns) if not self.is_protected(p))
        return sorted(i for _, i in cand[: len(conns) - low_water])


def topic_tag(topic):
    return f"pubsub:{topic}"


class TagTracer:
    def __init__(self, cmgr, params=None, direct=None):  # newTagTracer, :58-70
        self.cmgr, self.p = cmgr, params or Params()
        self.decaying = {}
        self.direct = direct  # a set, or None
        self.near_first = {}

    def tag_peer_if_direct(self, p):  # :81-91
        if self.direct is None:
            return
        if p in self.direct:
            self.cmgr.protect(p, "pubsub:<direct>")

    def add_delivery_tag(self, topic):  # :107-126
        try:
            tag = self.cmgr.register_decaying_tag(f"pubsub-deliveries:{topic}", 0, self.p.cap, self.p.decay_amount)
        except RuntimeError:
            return
        self.decaying[topic] = tag

    def remove_delivery_tag(self, topic):  # :128-140
        tag = self.decaying.get(topic)
        if tag is None:
            return
        tag.close()
        del self.decaying[topic]

    def bump_delivery_tag(self, p, topic):  # :142-151
        tag = self.decaying.get(topic)
        if tag is None:
            return False
        tag.bump(p, self.p.bump)
        return True

    # RawTracer
    def add_peer(self, p):  # :179-181
        self.tag_peer_if_direct(p)

    def join(self, topic):  # :183-185
        self.add_delivery_tag(topic)

    def leave(self, topic):  # :201-203
        self.remove_delivery_tag(topic)

    def graft(self, p, topic):  # :205-207
        self.cmgr.protect(p, topic_tag(topic))

    def prune(self, p, topic):  # :209-211
        self.cmgr.unprotect(p, topic_tag(topic))

    def validate_message(self, msg_id):  # :213-223
        if msg_id in self.near_first:
            return
        self.near_first[msg_id] = {}

    def duplicate_message(self, msg_id, received_from):  # :225-235
        peers = self.near_first.get(msg_id)
        if peers is None:
            return
        peers[received_from] = True

    def deliver_message(self, msg_id, received_from, topic):  # :187-199
        near = list(self.near_first.get(msg_id, {}))
        self.bump_delivery_tag(received_from, topic)
        for p in near:
            self.bump_delivery_tag(p, topic)
        self.near_first.pop(msg_id, None)

    def reject_message(self, msg_id, reason):  # :237-252
        if reason in (REJECT_THROTTLED, REJECT_IGNORED, REJECT_FAILED):
            self.near_first.pop(msg_id, None)

    # what the engine exports
    def delivery_value(self, p, topic):
        return self.cmgr.tag_value(p, f"pubsub-deliveries:{topic}")


# ---- the reference's own tests (tag_tracer_test.go) as runs over any backend ---------
# A backend is one observer's tracer: join / leave(topic), set_direct(peers),
# add_peer(p), graft / prune(p, topic), validate / duplicate / deliver(p, msg,
# topic), decay(steps), value(p, topic), mesh_protected(p), direct_protected(p).


class ModelBackend:
    def __init__(self, params=None):
        self.cm = ConnManager()
        self.tt = TagTracer(self.cm, params)

    def join(self, topic):
        self.tt.join(topic)

    def leave(self, topic):
        self.tt.leave(topic)

    def set_direct(self, peers):
        self.tt.direct = set(peers)

    def add_peer(self, p):
        self.tt.add_peer(p)

    def graft(self, p, topic):
        self.tt.graft(p, topic)

    def prune(self, p, topic):
        self.tt.prune(p, topic)

    def validate(self, p, msg, topic):
        self.tt.validate_message(msg)

    def duplicate(self, p, msg, topic):
        self.tt.duplicate_message(msg, p)

    def deliver(self, p, msg, topic):
        self.tt.deliver_message(msg, p, topic)

    def decay(self, steps):
        self.cm.tick(steps)

    def value(self, p, topic):
        return self.tt.delivery_value(p, topic)

    def mesh_protected(self, p):
        return any(t != "pubsub:<direct>" for t in self.cm.protected.get(p, ()))

    def direct_protected(self, p):
        return self.cm.is_protected(p, "pubsub:<direct>")


def kat_mesh_tags(be):  # TestTagTracerMeshTags
    be.join(0)
    be.graft(1, 0)
    a = be.mesh_protected(1)
    be.prune(1, 0)
    return {"after_graft": a, "after_prune": be.mesh_protected(1)}


def kat_direct_peer_tags(be):  # TestTagTracerDirectPeerTags
    be.set_direct([1])
    for p in (1, 2, 3):
        be.add_peer(p)
    return {"direct": [be.direct_protected(p) for p in (1, 2, 3)]}


def kat_delivery_tags(be, kat):  # TestTagTracerDeliveryTags, on a simulated clock
    be.join(0)
    be.join(1)
    for i in range(kat["deliveries"]):
        be.deliver(1, 100 + i, 1 if i < kat["to_second_topic"] else 0)
    out = {"values": [be.value(1, 0), be.value(1, 1)]}
    be.decay(kat["intervals"])
    out["values_after"] = [be.value(1, 0), be.value(1, 1)]
    be.leave(0)
    out["after_leave"] = be.value(1, 0)
    return out


def kat_near_first(be, kat):  # TestTagTracerDeliveryTagsNearFirst
    be.join(0)
    for i in range(kat["messages"]):
        be.validate(1, 500 + i, 0)
        be.duplicate(2, 500 + i, 0)  # before validation is complete: near-first
        be.deliver(1, 500 + i, 0)
        be.duplicate(3, 500 + i, 0)  # after it: no credit
    return {"values": [be.value(p, 0) for p in (1, 2, 3)]}


def run_kat(make_backend, kat):
    """-> {test name: what the backend gave}, to compare with kat[name]["expect"]."""
    return {
        "TestTagTracerMeshTags": kat_mesh_tags(make_backend()),
        "TestTagTracerDirectPeerTags": kat_direct_peer_tags(make_backend()),
        "TestTagTracerDeliveryTags": kat_delivery_tags(make_backend(), kat["TestTagTracerDeliveryTags"]),
        "TestTagTracerDeliveryTagsNearFirst": kat_near_first(make_backend(), kat["TestTagTracerDeliveryTagsNearFirst"]),
    }
