"""CPU checks of the junk-vote cases (tests/junk_vote_cases.py, run on the GPU
by tests/test_junk_votes_gpu.py): the C oracle and the statement-level
restatement agree on them (raft_election.go:54-77: votedFor outside [-1, P)
equals no candidate), the rule "kept while the term does not rise, cleared or
replaced when it does" holds in the oracle's election rounds and in the
model's clock steps, and the cases contain both outcomes."""
import numpy as np
import pytest

from junk_vote_cases import (JUNK_CASES, JUNK_G, JUNK_L, is_junk, junk_clock_model, junk_outcomes, junk_vote_case,
                             junk_values, py_election_rounds)
from oracle_lib import Oracle, assert_states_equal
from timers_cases import NOW0

from multiraft_amd import copy_state


def test_junk_values_are_outside_the_vote_domain():
    for P in (3, 5, 8):
        assert is_junk(junk_values(P), P).all()
        assert not is_junk(np.arange(-1, P), P).any()


@pytest.mark.parametrize("P,R", JUNK_CASES)
def test_election_rounds_junk_votes_c_vs_py(P, R):
    G, L = JUNK_G, JUNK_L
    st, mask = junk_vote_case(P, R)
    assert is_junk(st["voted_for"], P).sum() >= G * P // 6
    o = Oracle(G, P, L, st)
    gf = o.election_rounds(mask)
    pst, pgf = py_election_rounds(st, G, P, L, mask)
    assert np.array_equal(gf, pgf)
    assert_states_equal(o.state(), pst, G, P, L, f"junk votes, P {P} R {R}", heads=False)
    kept, changed = junk_outcomes(st, o.state(), P)
    assert kept >= 5 and changed >= 5, (kept, changed)


@pytest.mark.parametrize("P", [3, 5, 8])
def test_clock_steps_junk_votes_model(P):
    G, L = JUNK_G, JUNK_L
    st, _ = junk_vote_case(P, 1)
    m = junk_clock_model(P, st)
    kept = changed = 0
    for k in range(3):
        before = copy_state(m.state())
        m.clock_step(NOW0 + k, bool(k % 2))
        a, b = junk_outcomes(before, m.state(), P)
        kept, changed = kept + a, changed + b
    assert kept >= 5 and changed >= 5, (kept, changed)
    assert m.stats["grants"] and m.stats["elected"]
