"""CPU checks of the timers (include/mraft.h "timers"): the draw's known
answers through the library's host entry point and through the numpy model
(tests/timers_model.py), its range, the configurations it rejects, and the
model's self-driving runs — from Make state, clock steps alone elect one
Leader per group within two election timeouts and keep it (test_test.go
TestInitialElection), a crashed Leader is replaced at a higher term
(TestReElection), and Started entries commit."""
import numpy as np
import pytest

from multiraft_amd import _abi, features, timer_draw
from timers_model import (SELF_CFG, SELF_L, SELF_SHAPES, ModelNode, TimersModel, draw, fmix, self_driving)

KNOWN = [((0, 0, 0, 30, 60), 30), ((1, 0, 0, 30, 60), 37), ((1, 1, 0, 30, 60), 32), ((1, 0, 1, 30, 60), 53),
         ((0xdeadbeef, 327679, 1000000, 30, 60), 44), ((7, 12, 345, 300, 600), 556)]


def test_features_and_abi_version():
    assert features() & _abi.FEATURE_TIMERS
    assert _abi.lib().mraft_abi_version() == 6


def test_fmix_known_answers():
    assert int(fmix(1)) == 0x514e28b7
    assert int(fmix(2)) == 0x30f4c306
    assert int(fmix(0xffffffff)) == 0x81f16f39


@pytest.mark.parametrize("args,want", KNOWN)
def test_draw_known_answers(args, want):
    assert timer_draw(*args) == want
    assert int(draw(*args)) == want


def test_draws_in_range_and_equal_to_the_model():
    slots = np.arange(4096)
    for now in (0, 1, 77, 1 << 30):
        got = np.array([timer_draw(1, int(s), now, 30, 60, heartbeat=9) for s in slots])
        assert got.min() >= 30 and got.max() < 60
        assert np.array_equal(got, draw(1, slots, now, 30, 60))
    assert len(np.unique(got)) == 30  # every value of the range is drawn


@pytest.mark.parametrize("kw", [dict(heartbeat=0), dict(heartbeat=1 << 30), dict(election_lo=0), dict(election_lo=60),
                                dict(election_lo=61), dict(election_hi=(1 << 20) + 1), dict(now=-1),
                                dict(now=(1 << 30) + 1), dict(slot=-1), dict(slot=1 << 31)])
def test_bad_configurations_are_rejected(kw):
    a = dict(seed=1, slot=0, now=0, election_lo=30, election_hi=60, heartbeat=9)
    assert timer_draw(**a) == 37
    a.update(kw)
    with pytest.raises(ValueError):
        timer_draw(**a)
    assert _abi.lib().mraft_timer_draw(None, 0, 0) == -1


def test_draw_accepts_the_limits():
    assert 1 <= timer_draw(3, (1 << 31) - 1, 1 << 30, 1, 1 << 20, heartbeat=(1 << 30) - 1) < (1 << 20)


def test_model_ticker_cut_lists_keep_the_rest_due():
    """The buffer convention of mraft_ticker in the model: a listed slot that
    does not fit keeps its due timer, and the next call returns exactly the
    rest (the GPU tests compare the engine's cut lists with these)."""
    G, P = 40, 3
    gp = G * P
    for cap in (0, 1, 7, gp):
        m = TimersModel(G, P, 8)
        m.o.st["state"][::4] = _abi.LEADER
        m.enable(1, 9, 30, 60, 0)
        m.load(np.where(np.arange(gp) % 3 == 0, 101, 100).astype(np.int32), np.full(gp, 100, np.int32))
        leader = m.o.st["state"] == _abi.LEADER
        full_e, full_h = np.nonzero((m.ed <= 100) & ~leader)[0], np.nonzero(leader)[0]
        e1, ne, h1, nh = m.ticker(100, cap, cap)
        assert (ne, nh) == (len(full_e), len(full_h))
        assert np.array_equal(e1, full_e[:cap]) and np.array_equal(h1, full_h[:cap])
        assert (m.ed[full_e[cap:]] <= 100).all() and (m.ed[full_e[:cap]] > 100).all()
        assert (m.hd[full_h[cap:]] <= 100).all() and (m.hd[full_h[:cap]] > 100).all()
        assert (m.hd[~leader] == 109).all()           # a non-leader's due heartbeat timer is reset, never listed
        e2, ne2, h2, nh2 = m.ticker(100)
        assert np.array_equal(e2, full_e[cap:]) and np.array_equal(h2, full_h[cap:])
        assert m.ticker(100)[1::2] == (0, 0)


# The first tick at which every group has exactly one Leader. With P = 2 the
# last group is 25: its two replicas draw the same first deadline (46), both
# stand at tick 46 and refuse each other, and their resets at 46 draw 39 and 41,
# so replica 0 stands alone at tick 85 and wins.
FIRST_ALL_ONE_LEADER = {(64, 3): 52, (64, 5): 44, (64, 2): 85}


@pytest.mark.parametrize("G,P", SELF_SHAPES)
def test_model_self_driving_run(G, P):
    m = TimersModel(G, P, SELF_L)
    m.enable(SELF_CFG["seed"], SELF_CFG["heartbeat"], SELF_CFG["lo"], SELF_CFG["hi"], 0)
    hist = self_driving([ModelNode(m)], G, P)
    hi2 = 2 * SELF_CFG["hi"]
    if P == 1:
        # the reference counts votes only on a reply (raft_election.go:22-47): a
        # single replica times out for ever and is never elected
        assert all(h[0].sum() == 0 for h in hist.values())
        assert hist[420][1].min() > hist[120][1].max() > 0
        return
    first = min(t for t in range(1, 301) if (hist[t][0] == 1).all())
    assert first == FIRST_ALL_ONE_LEADER[(G, P)]
    for t in range(hi2, 301):
        assert (hist[t][0] == 1).all(), t
        assert np.array_equal(hist[t][1], hist[hi2][1]), f"a term changed at tick {t}"
        assert not hist[t][3].any(), f"an election at tick {t}"
    # leg 2: every Leader crashed at tick 300; by 300 + 2 * election_hi every
    # group has one Leader again, at a higher term
    t2 = 300 + hi2
    assert (hist[t2][0] == 1).all()
    st = m.state()
    lead = st["state"].reshape(G, P) == _abi.LEADER
    new_term = (st["current_term"].reshape(G, P) * lead).max(axis=1)
    assert (new_term > hist[300][1].reshape(G, P).max(axis=1)).all()
    # leg 3: the Started entries commit (the last Start is at least one tick
    # before the end), one Leader per group throughout
    t3 = max(hist)
    assert all((hist[t][0] == 1).all() for t in range(t2, t3 + 1))
    sl = np.nonzero(lead.reshape(-1))[0]
    assert (st["last_index"][sl] > 0).all()
    assert np.array_equal(st["commit_index"][sl], st["last_index"][sl])
    assert np.array_equal(hist[t3][2], st["commit_index"][sl])
