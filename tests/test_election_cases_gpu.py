"""The exhaustive, directed and edge cases of the election round
(tests/election_cases.py; their cells are proved present by
tests/test_election_cases.py) on libmraft_hip.so against the CPU oracle, bit
for bit, through the C ABI: mraft_election_rounds (group flags, the whole
state and the persist bits after a launch and after a second launch on what
the first left; R rounds in one launch against R launches of one; R = 0; a
null group_flags), mraft_clock_step on the same states with the timers loaded
so that round 0's mask falls due (k_clock_round compiles the same round body),
and the message-level round (mraft_start_election, mraft_handle_request_vote
per candidate rank, mraft_process_vote_replies) call by call, whose state must
also equal mraft_election_rounds on a second engine."""
import numpy as np
import pytest

import election_cases as ec
from oracle_lib import Oracle, assert_states_equal
from timers_cases import CFG, NOW0
from timers_model import compose_round

from multiraft_amd import Engine, _abi
from multiraft_amd._abi import HOST, ptr

pytestmark = pytest.mark.gpu

BIG = ec.BASES[1]


def run_rounds(case, R=None, dirty=None, launches=2):
    """`launches` launches of the case's first R rounds on one engine next to
    the oracle: flags, state and collect_persist equal after each."""
    G, P, L = case["G"], case["P"], case["L"]
    st = case["st"] if dirty is None else ec.with_dirty(case, dirty)
    mask = case["mask"] if R is None else case["mask"][:R]
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        for k in range(launches):
            ctx = f"{case['name']}, R {len(mask)}, launch {k}"
            gf = e.election_rounds(mask)
            assert np.array_equal(gf, o.election_rounds(mask)), ctx
            ec.assert_images_equal(e.store_state(), o.state(), G, P, L, ctx)
            assert np.array_equal(e.collect_persist(), o.collect_persist()), (ctx, "persist bits")


# ---- mraft_election_rounds ---------------------------------------------------------------------
@pytest.mark.parametrize("P,B,dirty", [(1, 10, None), (2, 10, None), (2, 10, 0xD1), (2, BIG, 0xD2), (3, 10, 0xD3)])
def test_exhaustive_rounds_gpu(P, B, dirty):
    run_rounds(ec.exhaustive(P, B), dirty=dirty)


@pytest.mark.parametrize("B", ec.BASES)
@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_directed_rounds_gpu(P, B):
    case = ec.directed(P, B)
    for R, dirty in ((1, None), (2, 0xD4 + P), (3, None)):
        run_rounds(case, R=R, dirty=dirty)


@pytest.mark.parametrize("P,G,L,R", ec.EDGE_CASES)
def test_edge_rounds_gpu(P, G, L, R):
    run_rounds(ec.edge(P, G, L, R), dirty=(0xD5 if (G + R) % 2 else None))


def test_rounds_in_one_launch_equal_single_round_launches_gpu():
    """Metamorphic, on the exhaustive P = 3 set: R rounds in one launch and R
    launches of one round leave the same state, persist bits and OR of flags."""
    case = ec.exhaustive(3)
    G, P, L, mask = case["G"], case["P"], case["L"], case["mask"]
    with Engine(G, P, L) as a, Engine(G, P, L) as b:
        a.load_state(case["st"])
        b.load_state(case["st"])
        gfa = a.election_rounds(mask)
        gfb = np.zeros(G, np.int32)
        for r in range(len(mask)):
            gfb |= b.election_rounds(mask[r:r + 1])
        assert np.array_equal(gfa, gfb)
        ec.assert_images_equal(a.store_state(), b.store_state(), G, P, L, "one launch / one launch per round")
        assert np.array_equal(a.collect_persist(), b.collect_persist())


@pytest.mark.parametrize("name", ["exhaustive 2", "directed 5", "edge"])
def test_zero_rounds_and_null_flags_gpu(name):
    case = {"exhaustive 2": lambda: ec.exhaustive(2), "directed 5": lambda: ec.directed(5),
            "edge": lambda: ec.edge(3, 65, ec.L_SMALL, 3)}[name]()
    G, P, L, mask = case["G"], case["P"], case["L"], case["mask"]
    st = ec.with_dirty(case, 0xD6)
    lib = _abi.lib()
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
        ed, hd = e.timers_store()
        # R = 0: nothing changes, flags 0
        gf = np.full(G, -1, np.int32)
        assert lib.mraft_election_rounds(e._h, ptr(mask), 0, ptr(gf), HOST) == 0, _abi.last_error()
        assert not gf.any()
        got = e.store_state()
        assert_states_equal(got, o.state(), G, P, L, f"{name}: R = 0")
        assert np.array_equal(got["persist_dirty"], st["persist_dirty"])
        for x, y in zip(e.timers_store(), (ed, hd)):
            assert np.array_equal(x, y)
        # group_flags == NULL: the same state as the run with flags
        assert lib.mraft_election_rounds(e._h, ptr(mask), len(mask), None, HOST) == 0, _abi.last_error()
        o.election_rounds(mask)
        assert_states_equal(e.store_state(), o.state(), G, P, L, f"{name}: null group_flags")
        assert np.array_equal(e.collect_persist(), o.collect_persist())


# ---- mraft_clock_step ---------------------------------------------------------------------------
def run_clock(case, send_all):
    G, P, L = case["G"], case["P"], case["L"]
    m = ec.clock_model(case)
    ed, hd = m.timers()
    with Engine(G, P, L) as e:
        e.load_state(case["st"])
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
        e.timers_load(ed, hd)
        for k in range(ec.CLOCK_STEPS):
            ctx = f"{case['name']}, send_all {send_all}, clock step {k}"
            want = m.clock_step(NOW0 + k, send_all)
            got = e.clock_step(NOW0 + k, send_all)
            for n in ec.CLOCK_OUTS:
                assert np.array_equal(got[n], want[n]), (ctx, n)
            assert_states_equal(e.store_state(), m.state(), G, P, L, ctx)
            for name, a, b in zip(("election_due", "heartbeat_due"), e.timers_store(), (m.ed, m.hd)):
                assert np.array_equal(a, b), (ctx, name)


@pytest.mark.parametrize("send_all", [False, True])
@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_clock_steps_directed_gpu(P, send_all):
    run_clock(ec.directed(P), send_all)


@pytest.mark.parametrize("send_all", [False, True])
def test_clock_steps_exhaustive_subset_gpu(send_all):
    run_clock(ec.exhaustive_subset(3, ec.CLOCK_SUBSET, seed=0xC10C), send_all)


# ---- the message-level round ----------------------------------------------------------------------
def run_message_rounds(case, rounds=2):
    """Rounds 0 and 1 composed from the three message-level calls on an Engine
    and on the Oracle in lockstep (every output and the state after each
    call), and mraft_election_rounds on a second engine."""
    G, P, L = case["G"], case["P"], case["L"]
    o = Oracle(G, P, L, case["st"])
    with Engine(G, P, L) as e, Engine(G, P, L) as fused:
        e.load_state(case["st"])
        fused.load_state(case["st"])
        for r in range(rounds):
            ctx = f"{case['name']}, message-level round {r}"
            node = ec.Lockstep(e, o, assert_states_equal, ctx)
            gf, _, _ = compose_round(node, G, P, ec.candidates_of(o.state(), case["mask"][r], P))
            assert node.calls >= 2 or P < 2 or not case["mask"][r].any()
            assert np.array_equal(fused.election_rounds(case["mask"][r:r + 1]), gf), ctx
            assert_states_equal(e.store_state(), fused.store_state(), G, P, L, ctx + " against election_rounds")
            pb = o.collect_persist()
            assert np.array_equal(e.collect_persist(), pb) and np.array_equal(fused.collect_persist(), pb), ctx


@pytest.mark.parametrize("B", ec.BASES)
@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_message_level_round_directed_gpu(P, B):
    run_message_rounds(ec.directed(P, B))


@pytest.mark.parametrize("B", ec.BASES)
def test_message_level_round_exhaustive_gpu(B):
    run_message_rounds(ec.exhaustive(2, B))
