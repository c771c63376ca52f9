"""The Python model of tag_tracer.go (tests/tag_model.py) reproduces the values
the reference's own tests assert (tests/golden/tag_kat.json), and its trim
follows the contract of gsx_conn_trim."""
import json
import os

import tag_model as tm

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tag_kat.json")))


def test_model_reproduces_the_reference_tests():
    p = KAT["params"]
    got = tm.run_kat(lambda: tm.ModelBackend(tm.Params(p["bump"], p["decay_amount"], p["cap"], p["decay_interval_ns"])), KAT)
    for name, g in got.items():
        assert g == KAT[name]["expect"], name


def test_bump_at_an_unjoined_topic_fails_and_the_entry_is_still_deleted():
    be = tm.ModelBackend()
    be.validate(1, 7, 0)
    be.duplicate(2, 7, 0)
    be.deliver(1, 7, 0)
    assert be.value(1, 0) == 0 and be.value(2, 0) == 0 and not be.tt.near_first


def test_reject_deletes_the_entry_for_the_validation_reasons_only():
    be = tm.ModelBackend()
    be.validate(1, 7, 0)
    be.tt.reject_message(7, "missing signature")
    assert 7 in be.tt.near_first
    be.tt.reject_message(7, tm.REJECT_IGNORED)
    assert not be.tt.near_first


def test_trim_contract():
    cm = tm.ConnManager()
    tag = cm.register_decaying_tag("x", 0, 15, 1)
    for p, v in enumerate([3, 0, 3, 1, 0, 9]):
        if v:
            tag.bump(p, v)
    cm.protect(1, "pubsub:t")
    conns = [0, 1, 2, 3, 4, 5]
    assert cm.trim(conns, 6) == [] and cm.trim(conns, 9) == []
    assert cm.trim(conns, 4) == [3, 4]        # values 0 (peer 4), 1 (peer 3); peer 1 is protected
    assert cm.trim(conns, 3) == [0, 3, 4]     # the tie at 3: the lower index goes first
    assert cm.trim(conns, 0) == [0, 2, 3, 4, 5]  # never a protected one
