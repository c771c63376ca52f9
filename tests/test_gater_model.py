"""CPU checks of the peer gater: the model (tests/gater_model.py) passes the
reference's TestPeerGater (peer_gater_test.go:11-128) restated on a simulated
clock, and the library's host-side gsx_validate_gater_params /
gsx_default_gater_params agree with PeerGaterParams.validate
(peer_gater.go:57-88) and DefaultPeerGaterParams (:19-28, 98-116).  No device
work."""
import ctypes as C

import pytest

import gater_model as gm
import gsx
from gsx import abi

SEED = 0x9A7E5


def test_model_passes_TestPeerGater():
    now = 1_700_000_000 * abi.SECOND
    params = gm.Params(0.1, 0.9, 0.999)  # NewPeerGaterParams(.1, .9, .999)
    assert params.validate() is None
    pg = gm.PeerGater(params, lambda p: "1.2.3.4" if p == "A" else "<wtf>")
    draw = [0]

    def accept():
        draw[0] += 1
        return pg.accept_from("A", now, gm.canonical_u(SEED, 0, draw[0] - 1))

    pg.add_peer("A")
    assert accept() == gm.ACCEPT_ALL
    pg.validate_message()
    assert accept() == gm.ACCEPT_ALL
    pg.reject_message("A", gm.REJECT_QUEUE_FULL, now)
    assert accept() == gm.ACCEPT_ALL
    pg.reject_message("A", gm.REJECT_THROTTLED, now)
    assert accept() == gm.ACCEPT_ALL
    for _ in range(100):
        pg.reject_message("A", gm.REJECT_IGNORED, now)
        pg.reject_message("A", gm.REJECT_FAILED, now)
    # "within 1000 tries": draws 0..999 of the fixed seed
    assert any(pg.accept_from("A", now, gm.canonical_u(SEED, 0, k)) == gm.ACCEPT_CONTROL for k in range(1000))
    for _ in range(100):
        pg.deliver_message("A", "")
    assert any(pg.accept_from("A", now, gm.canonical_u(SEED, 0, k)) == gm.ACCEPT_ALL for k in range(1000))
    for _ in range(100):
        now += params.decay_interval
        pg.decay_stats(now)
    assert accept() == gm.ACCEPT_ALL
    pg.remove_peer("A", now)
    assert "A" not in pg.peer_stats
    assert "1.2.3.4" in pg.ip_stats
    pg.ip_stats["1.2.3.4"].expire = now
    now += 2 * abi.SECOND  # time.Sleep(2 * time.Second): the ticker ran
    pg.decay_stats(now)
    assert "1.2.3.4" not in pg.ip_stats


def test_canonical_draw_is_a_53_bit_fraction():
    us = [gm.canonical_u(SEED, p, d) for p in range(20) for d in range(20)]
    assert all(0.0 <= u < 1.0 and (u * 2.0 ** 53).is_integer() for u in us)
    assert len(set(us)) == len(us)
    assert 0.4 < sum(us) / len(us) < 0.6


def _valid():
    p = abi.GaterParams()
    assert gsx.load_library().gsx_default_gater_params(C.byref(p)) == 0
    return p


def test_default_gater_params():
    lib = gsx.load_library()
    p = _valid()
    assert lib.gsx_validate_gater_params(C.byref(p)) == 0
    assert p.threshold == 0.33
    assert p.global_decay == lib.gsx_score_parameter_decay(2 * abi.MINUTE)
    assert p.source_decay == lib.gsx_score_parameter_decay(abi.HOUR)
    assert p.decay_interval_ns == abi.SECOND and p.decay_to_zero == 0.01
    assert p.retain_stats_ns == 6 * abi.HOUR and p.quiet_ns == abi.MINUTE
    assert (p.duplicate_weight, p.ignore_weight, p.reject_weight) == (0.125, 1.0, 16.0)
    assert all(w == 0.0 for w in p.topic_delivery_weight)
    m = gm.Params(p.threshold, p.global_decay, p.source_decay)
    assert m.validate() is None
    assert lib.gsx_validate_gater_params(None) == abi.GSX_EINVAL
    assert lib.gsx_default_gater_params(None) == abi.GSX_EINVAL


# one violating value per rule of peer_gater.go:57-88 (field, value, model attribute)
VIOLATIONS = [
    ("threshold", 0.0, "threshold"),
    ("global_decay", 0.0, "global_decay"),
    ("global_decay", 1.0, "global_decay"),
    ("source_decay", 0.0, "source_decay"),
    ("source_decay", 1.0, "source_decay"),
    ("decay_interval_ns", abi.SECOND - 1, "decay_interval"),
    ("decay_to_zero", 0.0, "decay_to_zero"),
    ("decay_to_zero", 1.0, "decay_to_zero"),
    ("quiet_ns", abi.SECOND - 1, "quiet"),
    ("duplicate_weight", 0.0, "duplicate_weight"),
    ("ignore_weight", 0.5, "ignore_weight"),
    ("reject_weight", 0.5, "reject_weight"),
]


@pytest.mark.parametrize("field,value,attr", VIOLATIONS, ids=[f"{f}={v}" for f, v, _ in VIOLATIONS])
def test_validate_gater_params(field, value, attr):
    lib = gsx.load_library()
    p = _valid()
    setattr(p, field, value)
    assert lib.gsx_validate_gater_params(C.byref(p)) == abi.GSX_EINVAL
    m = gm.Params(0.33, 0.5, 0.5)
    setattr(m, attr, value)
    assert m.validate() is not None


def test_retention_is_not_validated():
    p = _valid()
    p.retain_stats_ns = 0  # "a value of 0 means we don't retain stats"
    assert gsx.load_library().gsx_validate_gater_params(C.byref(p)) == 0
