"""CPU check of the model at the top of the time domain
(tests/time_domain_cases.py, run on the GPU by tests/test_time_domain_gpu.py):
the model's own deadlines stay within int32 for these inputs — so the model is
not what wraps — and its compares are right for loaded deadlines at INT32_MIN
and INT32_MAX."""
import numpy as np
import pytest

from time_domain_cases import (INT32_MAX, TOP_CFG, TOP_G, TOP_L, TOP_NOWS, TOP_P, edge_values, top_of_time_run,
                               top_state)
from timers_model import ModelNode, TimersModel, draw

from multiraft_amd._abi import LEADER


def check_model(m, nows):
    """Every deadline of the model is the value last loaded into its slot or a
    reset at one of the run's `nows`, and the resets are recomputed here in
    Python integers: now + heartbeat, or now + the one draw of the range —
    none above 2^31 - 1. Before the first load every deadline is a reset."""
    hb, lo, hi = TOP_CFG["heartbeat"], TOP_CFG["election_lo"], TOP_CFG["election_hi"]
    assert hi == lo + 1  # the draw is lo
    resets_e, resets_h = [t + lo for t in nows], [t + hb for t in nows]
    assert max(resets_e + resets_h) <= INT32_MAX and TOP_NOWS[-1] + hb == INT32_MAX

    def check(ctx, loaded):
        assert m.ed.dtype == np.int32 and m.hd.dtype == np.int32
        for name, due, resets, k in (("election_due", m.ed, resets_e, 0), ("heartbeat_due", m.hd, resets_h, 1)):
            due = due.astype(np.int64)
            own = np.ones(len(due), bool) if loaded is None else due != loaded[k].astype(np.int64)
            assert np.isin(due[own], resets).all(), (ctx, name, due[own][~np.isin(due[own], resets)][:8])
    return check


@pytest.mark.parametrize("now", TOP_NOWS)
def test_model_deadlines_stay_int32_at_the_top(now):
    m = TimersModel(TOP_G, TOP_P, TOP_L, top_state())
    top_of_time_run([ModelNode(m)], now, check_model(m, (now,)))
    # the draw itself, in Python integers
    slots = np.arange(TOP_G * TOP_P)
    d = draw(TOP_CFG["seed"], slots, now, TOP_CFG["election_lo"], TOP_CFG["election_hi"])
    assert d.dtype == np.int64 and (d == TOP_CFG["election_lo"]).all()  # a range of one value
    assert int(now + d.max()) <= INT32_MAX


def test_model_consecutive_clock_steps_up_to_the_last_tick():
    m = TimersModel(TOP_G, TOP_P, TOP_L, top_state())
    top_of_time_run([ModelNode(m)], TOP_NOWS[0], check_model(m, TOP_NOWS), clock_nows=TOP_NOWS)
    assert int(m.hd.max()) == INT32_MAX  # now + heartbeat at now = 2^30, or a loaded INT32_MAX


@pytest.mark.parametrize("now", TOP_NOWS)
def test_model_compares_at_the_int32_limits(now):
    """INT32_MIN, -1, 0, now - 1 and now are due at `now`; now + 1 and
    INT32_MAX are not."""
    st = top_state()
    m = TimersModel(TOP_G, TOP_P, TOP_L, st)
    m.enable(TOP_CFG["seed"], TOP_CFG["heartbeat"], TOP_CFG["election_lo"], TOP_CFG["election_hi"], now)
    gp = TOP_G * TOP_P
    vals = edge_values(now)
    ed = vals[np.arange(gp) % 7].astype(np.int32)
    hd = vals[(np.arange(gp) // 7) % 7].astype(np.int32)
    m.load(ed, hd)
    e, ne, h, nh = m.ticker(now)
    leader = st["state"] == LEADER
    assert np.array_equal(e, np.nonzero((np.arange(gp) % 7 < 5) & ~leader)[0])
    assert np.array_equal(h, np.nonzero(((np.arange(gp) // 7) % 7 < 5) & leader)[0])
    assert ne == len(e) > 0 and nh == len(h) > 0
    assert (m.ed[np.arange(gp) % 7 < 5] == now + TOP_CFG["election_lo"]).all()
    assert np.array_equal(m.ed[np.arange(gp) % 7 >= 5], ed[np.arange(gp) % 7 >= 5])
    assert (m.hd[(np.arange(gp) // 7) % 7 < 5] == now + TOP_CFG["heartbeat"]).all()
