"""The parameter table of gossipsub_param_cases.py through the oracle alone:
every case's counters prove that the branch it is about ran, so a case that
went dead is caught without a GPU.  Plus the oracle's rejected-draw counters
(oracle.rng_rejections), which tests/test_gpu_rng_rejection.py relies on."""
import pytest

import gossipsub_param_cases as gpc
import oracle as orc
import rejection_cases as rc


@pytest.mark.parametrize("name", list(gpc.EXCHANGE))
def test_exchange_case_is_live(name):
    _, outs, _, _ = gpc.exchange_case(orc.Oracle(2), name)
    gpc.EXCHANGE[name][1](outs)


def test_grow_case_is_live():
    gpc.grow_check(gpc.grow_run(orc.Oracle(2)))


def test_mesh_cases_are_live():
    grafts = {}
    for name in gpc.MESH:
        _, outs, _ = gpc.mesh_case(orc.Oracle(2), name)
        gpc.MESH[name][3](outs)
        grafts[name] = sum(o["grafts"] for o in outs)
    gpc.og_cross_check(grafts)


def test_hub_sort_case_is_live():
    gpc.hub_sort_check(gpc.hub_sort_run(orc.Oracle(2))[1])


def test_rejection_counters_reset_and_count():
    """Zero after a reset; AddPromise's pick among 1000 handles with a seed
    whose first draw is rejected (found from the hash) counts on tag 9."""
    seeds = rc.SEEDS["promise"]["seeds"]
    assert all(rc.promise_seed_rejects(s) > 0 for s in seeds)
    orc.rng_rejections_reset()
    assert orc.rng_rejections() == {}
    kept = rc.promise_run(orc.Oracle(1), seeds)
    assert orc.rng_rejections() == rc.SEEDS["promise"]["rej"]
    assert all(before == 1 and after == 0 for _, before, after in kept), kept
    orc.rng_rejections_reset()
    assert orc.rng_rejections() == {}
    rc.promise_run(orc.Oracle(1), [s for s in range(50) if not rc.promise_seed_rejects(s)][:5])
    assert orc.rng_rejections() == {}
