"""CPU checks of the reachability model and cases (tests/reach_model.py,
tests/reach_cases.py): the model equals the oracle wherever the oracle can
speak (every bit set), the hand-derived known answers, and what the built
cases contain. No GPU."""
import numpy as np
import pytest

import election_cases as ec
import reach_cases as rc
from oracle_lib import Oracle, assert_states_equal
from reach_model import connected, full_mask, masked_election_rounds, masked_tick
from timers_cases import CLOCK_CASES, CLOCK_STEPS, NOW0, clock_case_model

from multiraft_amd import _abi


# ---- 1. the model is the oracle at full mask ------------------------------------------------------
@pytest.mark.parametrize("kind", ["fuzz", "snap", "synth"])
@pytest.mark.parametrize("P", rc.TICK_P)
def test_model_tick_equals_oracle_at_full_mask(P, kind):
    for seed, G in enumerate(rc.TICK_G):
        st, lp, _, _ = rc.tick_case(P, G, seed, kind)
        L = rc.TICK_L
        o, m = Oracle(G, P, L, st), Oracle(G, P, L, st)
        for k in range(2):
            assert np.array_equal(masked_tick(m, lp, full_mask(G, P)), o.replicate_tick(lp)), (P, kind, G, k)
            assert_states_equal(m.state(), o.state(), G, P, L, f"P {P} {kind} G {G} tick {k}")
            for a, b in zip(m.export_group_status(lp), o.export_group_status(lp)):
                assert np.array_equal(a, b)


def _round_equal(case):
    G, P, L = case["G"], case["P"], case["L"]
    o, m = Oracle(G, P, L, case["st"]), Oracle(G, P, L, case["st"])
    assert np.array_equal(masked_election_rounds(m, case["mask"], full_mask(G, P)), o.election_rounds(case["mask"]))
    ec.assert_images_equal(m.state(), o.state(), G, P, L, case["name"])


@pytest.mark.parametrize("P", (1, 2))
def test_model_round_equals_oracle_exhaustive(P):
    _round_equal(ec.exhaustive(P))


@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_model_round_equals_oracle_directed(P):
    _round_equal(ec.directed(P))


@pytest.mark.parametrize("P,G,send_all", CLOCK_CASES)
def test_model_clock_equals_timers_model(P, G, send_all):
    L, st, ed, hd, want = clock_case_model(P, G, send_all)
    _, _, _, _, m = rc.clock_model(P, G, send_all)
    m.set_reachable(full_mask(G, P))
    for k in range(CLOCK_STEPS):
        a, b = m.clock_step(NOW0 + k, send_all), want.clock_step(NOW0 + k, send_all)
        for n in b:
            assert np.array_equal(a[n], b[n]), (P, G, send_all, k, n)
        assert_states_equal(m.state(), want.state(), G, P, L, "clock at full mask")
        assert np.array_equal(m.ed, want.ed) and np.array_equal(m.hd, want.hd)


# ---- 2. hand-derived known answers -----------------------------------------------------------------
@pytest.mark.parametrize("ka", rc.known_answers(), ids=lambda k: k["name"])
def test_known_answers_model(ka):
    o = Oracle(ka["G"], ka["P"], ka["L"], ka["st"])
    reach = np.array(ka["reach"], np.uint8)
    if ka["kind"] == "tick":
        gf = masked_tick(o, np.array(ka["lp"], np.int32), reach)
    else:
        gf = masked_election_rounds(o, np.array([ka["cand"]], np.uint8), reach)
    rc.check_known_answer(ka, gf, o.state())


# ---- 3. presence -----------------------------------------------------------------------------------
def test_tick_cases_contain_every_mask_and_reply_class():
    seen = {c: 0 for c in rc.TICK_CLASSES}
    cut = {}
    leaders = {P: set() for P in rc.TICK_P}
    for P in rc.TICK_P:
        for seed, G in enumerate(rc.TICK_G):
            for kind in ("fuzz", "snap"):
                st, lp, reach, cls = rc.tick_case(P, G, seed, kind)
                for c in cls:
                    seen[c] += 1
                leaders[P] |= {int(x) for x in lp if 0 <= x < P}
                for k, v in rc.undelivered_classes(st, G, P, rc.TICK_L, lp, reach).items():
                    cut[k] = cut.get(k, 0) + v
    assert all(v > 0 for v in seen.values()), seen
    # every reply class among the followers a mask cuts off: merge, heartbeat, conflict (the
    # scan), stale with a higher term, needs-snapshot and capacity-full
    assert all(cut[k] > 0 for k in ("merge", "heartbeat", "conflict", "stale", "snapshot", "log_full")), cut
    for P in rc.TICK_P:
        assert {0, P // 2, P - 1} <= leaders[P], (P, leaders[P])


def test_tick_mask_classes_mean_what_they_say():
    for P in rc.TICK_P:
        for lp in (0, P // 2, P - 1):
            full = (1 << P) - 1
            n = lambda c: bin(rc.tick_mask(c, P, lp, 1) & full).count("1")  # noqa: E731
            assert n("full") == P and n("leader_clear") == P - 1 and not rc.tick_mask("leader_clear", P, lp, 1) >> lp & 1
            assert n("majority") == P // 2 + 1 and n("one_short") == P // 2 and n("leader_plus_one") == 2
            assert rc.tick_mask("majority", P, lp, 1) >> lp & 1
            if P < 8:
                assert rc.tick_mask("high_bits", P, lp, 1) >> P


def test_chunk_edge_case_is_what_it_says():
    G, P, L, st, lp, reach = rc.chunk_edge_case()
    rec = {}
    o = Oracle(G, P, L, st)
    before = o.state()["last_index"].copy()
    gf = masked_tick(o, lp, reach, rec)
    assert (gf & _abi.G_ACTIVE).all() and not (gf & _abi.G_ERROR).any()
    assert (rec["delivered"].sum(axis=1) == 1).all()
    for g in range(G):
        near = 1 if g % 2 == 0 else 2
        far = 3 - near
        lo, hi = before[g * P + near] + 1, o.state()["last_index"][g * P + near]
        assert hi == before[g * P] and lo // 256 != hi // 256, "the merge crosses a 256-entry chunk edge"
        assert o.state()["last_index"][g * P + far] == before[g * P + far] == 39
        assert st["next_index"][g * P * P + far] < lo, "the follower cut off would have started lower"


def test_clock_masks_change_and_cut_leaders():
    cut_leader = partial = 0
    for P, G, sa in CLOCK_CASES:
        L, st, ed, hd = rc.clock_case(P, G, sa)
        ms = [rc.clock_masks(P, G, sa, k) for k in range(rc.CLOCK_STEPS // rc.CLOCK_MASK_EVERY)]
        assert G == 1 or not np.array_equal(ms[0], ms[1])
        conn = connected(ms[0], G, P).reshape(-1)
        cut_leader += int(((st["state"] == _abi.LEADER) & ~conn).sum())
        partial += int(((ms[0] & ((1 << P) - 1)) != (1 << P) - 1).sum())
    assert cut_leader > 100 and partial > 100


def test_scenario_schedules():
    """The schedules are test_test.go's: who is cut off in each phase."""
    P, sched = rc.SCENARIOS["ReElection2A"]
    masks = [fn(P, 1, 1) for fn, _ in sched]
    assert masks == [0b111, 0b101, 0b111, 0b001, 0b101, 0b111]
    P, sched = rc.SCENARIOS["FailNoAgree2B"]
    assert [fn(P, 0, 0) for fn, _ in sched] == [0b11111, 0b10001, 0b11111, 0b11111]
    P, sched = rc.SCENARIOS["FailAgree2B"]
    assert [fn(P, 2, 2) for fn, _ in sched] == [0b111, 0b110, 0b110, 0b111]
    P, sched = rc.SCENARIOS["Rejoin2B"]
    assert [fn(P, 0, 0) for fn, _ in sched][1] == 0b110
