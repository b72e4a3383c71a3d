"""The timer calls at the top of the time domain against the model
(tests/time_domain_cases.py): enable, arm, ticker, mraft_timers_note and the
clock step at now in {2^30 - 2, 2^30 - 1, 2^30} with heartbeat = 2^30 - 1 and
election range [2^20 - 1, 2^20), on loaded deadlines at INT32_MIN, INT32_MAX
and either side of `now`. now + draw and now + heartbeat must stay inside
int32 (the latter is 2^31 - 1 at now = 2^30) and the compares must hold at the
limits; tests/test_time_domain.py checks that the model does not wrap."""
import numpy as np
import pytest

from oracle_lib import assert_states_equal
from time_domain_cases import TOP_G, TOP_L, TOP_NOWS, TOP_P, top_of_time_run, top_state
from timers_model import ModelNode, TimersModel

from multiraft_amd import Engine

pytestmark = pytest.mark.gpu


def against_model(e, m):
    def check(ctx, loaded):
        assert_states_equal(e.store_state(), m.state(), TOP_G, TOP_P, TOP_L, ctx)
        for name, a, b in zip(("election_due", "heartbeat_due"), e.timers_store(), (m.ed, m.hd)):
            bad = np.nonzero(a != b)[0][:8]
            assert not len(bad), f"{ctx}: {name} differs at {bad}: {a[bad]} vs {b[bad]}"
    return check


@pytest.mark.parametrize("now", TOP_NOWS)
def test_timer_calls_at_the_top_of_the_time_domain(now):
    st = top_state()
    m = TimersModel(TOP_G, TOP_P, TOP_L, st)
    with Engine(TOP_G, TOP_P, TOP_L) as e:
        e.load_state(st)
        top_of_time_run([ModelNode(m), e], now, against_model(e, m))


def test_consecutive_clock_steps_up_to_the_last_tick():
    st = top_state()
    m = TimersModel(TOP_G, TOP_P, TOP_L, st)
    with Engine(TOP_G, TOP_P, TOP_L) as e:
        e.load_state(st)
        top_of_time_run([ModelNode(m), e], TOP_NOWS[0], against_model(e, m), clock_nows=TOP_NOWS)
