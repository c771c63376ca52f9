"""gsx_gossipsub_params away from DefaultGossipSubParams on the GPU vs the
oracle, bit for bit: the table of gossipsub_param_cases.py (d_lazy,
gossip_factor, gossip_retransmission, iwant_followup_ns, max_ihave_length 0
and 1, max_ihave_messages 1, history windows; mesh degrees at their edges,
opportunistic grafting counts, sub-second backoff).  Each case's counters
(from the oracle's run) prove its branch ran."""
import pytest

import gossipsub_param_cases as gpc
import gsx
import oracle as orc
from test_gpu_gossip import _same as _same_exchange
from test_gpu_heartbeat import _same as _same_state

pytestmark = pytest.mark.gpu


def _rounds_equal(g, w):
    (_, go, gs), (_, wo, ws) = g, w
    for k in range(len(wo)):
        assert go[k] == wo[k], (k, {f: (go[k][f], wo[k][f]) for f in wo[k] if go[k][f] != wo[k][f]})
        _same_state(gs[k], ws[k], f"tick {k}")


@pytest.mark.parametrize("name", list(gpc.EXCHANGE))
def test_exchange_params_match_oracle(gpu_ok, name):
    w = gpc.exchange_case(orc.Oracle(2), name)
    gpc.EXCHANGE[name][1](w[1])
    _same_exchange(gpc.exchange_case(gsx.Engine(2), name), w)


def test_targets_grow_between_rounds_then_fanout(gpu_ok):
    w = gpc.grow_run(orc.Oracle(2))
    gpc.grow_check(w)
    _rounds_equal(gpc.grow_run(gsx.Engine(2))[:3], w[:3])


@pytest.mark.parametrize("name", list(gpc.MESH))
def test_mesh_params_match_oracle(gpu_ok, name):
    w = gpc.mesh_case(orc.Oracle(2), name)
    gpc.MESH[name][3](w[1])
    _rounds_equal(gpc.mesh_case(gsx.Engine(2), name), w)


def test_hub_sort_then_empty_shuffle(gpu_ok):
    w = gpc.hub_sort_run(orc.Oracle(2))
    gpc.hub_sort_check(w[1])
    _rounds_equal(gpc.hub_sort_run(gsx.Engine(2)), w)
