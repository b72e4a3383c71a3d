"""votedFor outside [-1, P) on the GPU (tests/junk_vote_cases.py): the
election round's kVJunk path in mraft_election_rounds against the C oracle,
and in three clock steps against the model. The state is identical, so a junk
vote is kept while its voter's term does not rise and cleared or replaced when
it does (tests/test_junk_votes.py checks on the CPU that the cases contain
both outcomes)."""
import numpy as np
import pytest

from junk_vote_cases import JUNK_CASES, JUNK_G, JUNK_L, junk_clock_model, junk_outcomes, junk_vote_case
from oracle_lib import Oracle, assert_states_equal
from timers_cases import CFG, NOW0

from multiraft_amd import Engine

pytestmark = pytest.mark.gpu

OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


@pytest.mark.parametrize("P,R", JUNK_CASES)
def test_election_rounds_junk_votes_gpu(P, R):
    G, L = JUNK_G, JUNK_L
    st, mask = junk_vote_case(P, R)
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        gf = e.election_rounds(mask)
        assert np.array_equal(gf, o.election_rounds(mask))
        got = e.store_state()
        assert_states_equal(got, o.state(), G, P, L, f"junk votes, P {P} R {R}")
        kept, changed = junk_outcomes(st, got, P)
        assert kept and changed
        # a second launch on what the first left
        assert np.array_equal(e.election_rounds(mask), o.election_rounds(mask))
        assert_states_equal(e.store_state(), o.state(), G, P, L, f"junk votes, P {P} R {R}, second launch")


@pytest.mark.parametrize("P", [3, 5, 8])
def test_clock_steps_junk_votes_gpu(P):
    G, L = JUNK_G, JUNK_L
    st, _ = junk_vote_case(P, 1)
    m = junk_clock_model(P, st)
    ed, hd = m.timers()
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
        e.timers_load(ed, hd)
        for k in range(3):
            ctx = f"junk votes, P {P}, clock step {k}"
            want = m.clock_step(NOW0 + k, bool(k % 2))
            got = e.clock_step(NOW0 + k, bool(k % 2))
            for n in OUTS:
                assert np.array_equal(got[n], want[n]), (ctx, n)
            assert_states_equal(e.store_state(), m.state(), G, P, L, ctx)
            for name, a, b in zip(("election_due", "heartbeat_due"), e.timers_store(), (m.ed, m.hd)):
                assert np.array_equal(a, b), (ctx, name)
