"""mraft_clock_step against the host-driven sequence of the same tick
(tests/timers_sequence.py), on two engines that start from the same state and
timers: one runs clock_step, the other ticker, the message-level calls and
mraft_timers_note. The two engines agree wherever the equivalence is defined
(state, logs, persist bits and election_due equal in the inside groups, the
two documented heartbeat_due differences asserted), and each engine equals its
model counterpart in every group after every step."""
import numpy as np
import pytest

from oracle_lib import assert_states_equal
from timers_cases import CFG, CLOCK_STEPS, NOW0, clock_case
from timers_sequence import compare, lockstep, run_model_case

from multiraft_amd import Engine

pytestmark = pytest.mark.gpu

OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")
INFO = ("E", "H", "granted", "became", "stepped_down", "deposed", "leader_peer", "n_eligible")


@pytest.mark.parametrize("send_all", [False, True])
@pytest.mark.parametrize("P,G", [(2, 300), (3, 33), (5, 33), (5, 300), (8, 300)])
def test_clock_step_equals_the_host_driven_sequence_gpu(P, G, send_all):
    ctx = f"P {P} G {G} send_all {send_all}"
    L, st, ed, hd = clock_case(P, G, send_all)
    want, want_stats = run_model_case(P, G, send_all)
    with Engine(G, P, L) as e1, Engine(G, P, L) as e2:
        for e in (e1, e2):
            e.load_state(st)
            e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
            e.timers_load(ed, hd)
        got = lockstep(e1, e2, NOW0, CLOCK_STEPS, send_all)
    # each engine against its model counterpart, every group, every step
    for k, (g, w) in enumerate(zip(got, want)):
        for n in OUTS:
            assert np.array_equal(g["out"][n], w["out"][n]), (ctx, k, n)
        for n in INFO:
            assert np.array_equal(g["info"][n], w["info"][n]), (ctx, k, n)
        for side in ("clock", "seq"):
            assert_states_equal(g[side][0], w[side][0], G, P, L, f"{ctx} step {k}, {side} side against its model")
            for name, a, b in zip(("election_due", "heartbeat_due"), g[side][1:], w[side][1:]):
                bad = np.nonzero(a != b)[0][:8]
                assert not len(bad), f"{ctx} step {k}, {side} side: {name} differs at {bad}: {a[bad]} vs {b[bad]}"
    # the two engines against each other
    stats = compare(got, G, P, L, CFG["heartbeat"], ctx)
    assert stats == want_stats
    assert stats["inside"] > 0
