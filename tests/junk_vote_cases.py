"""Seeded election states whose votedFor is outside [-1, P) in a third of the
non-leader slots: the kVJunk path of the election round (k_election_rounds
and, as shared text, k_clock_round). HandleRequestVote (raft_election.go:54-77)
grants only when votedFor is -1 or the candidate, so such a vote matches no
candidate: it is kept while the voter's term does not rise, and cleared to -1
(then possibly given to a candidate) or replaced by the replica's own id
(StartElection, :4-15) when it does. Test infrastructure only."""
from __future__ import annotations

import os
import sys

import numpy as np

from multiraft_amd import synth_election_state
from multiraft_amd._abi import G_ELECTED, G_STEPPED_DOWN, LEADER
from timers_cases import CFG, NOW0, due_timers
from timers_model import TimersModel

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
JUNK_G, JUNK_L = 64, 16
JUNK_CASES = [(P, R) for P in (3, 5, 8) for R in (1, 4)]


def junk_values(P):
    return np.array([P, 8, 100, -2, INT32_MIN, INT32_MAX], dtype=np.int64)


def is_junk(voted, P):
    v = np.asarray(voted, dtype=np.int64)
    return (v < -1) | (v >= P)


def junk_vote_case(P, R):
    """(state, cand_mask[R, G]): random candidate masks, about a third of the
    replicas timing out per round; a quarter of the groups stay quiet, so
    their junk votes meet no higher term in any round."""
    G, L = JUNK_G, JUNK_L
    rng = np.random.default_rng(7700 + 10 * P + R)
    st, _ = synth_election_state(G, P, L, seed=7700 + 10 * P + R, rounds=1)
    pick = (st["state"] != LEADER) & (rng.random(G * P) < 1 / 3)
    st["voted_for"][pick] = rng.choice(junk_values(P), size=int(pick.sum())).astype(np.int32)
    bits = ((rng.random((R, G, P)) < 0.3) & (rng.random(G) >= 0.25)[None, :, None]).astype(np.uint8)
    mask = (bits << np.arange(P, dtype=np.uint8)).sum(axis=2).astype(np.uint8)
    return st, mask


def junk_outcomes(before, after, P):
    """Of the slots that held a junk vote: (kept, cleared or replaced) counts.
    Asserts the rule: kept exactly when the term did not rise, and otherwise a
    vote in [-1, P)."""
    j = is_junk(before["voted_for"], P)
    rose = after["current_term"] > before["current_term"]
    assert not (after["current_term"] < before["current_term"]).any()
    assert np.array_equal(after["voted_for"][j & ~rose], before["voted_for"][j & ~rose]), \
        "a junk vote changed at an unchanged term"
    assert not is_junk(after["voted_for"][j & rose], P).any(), "a junk vote survived a term change"
    assert not is_junk(after["voted_for"][~j], P).any(), "a junk vote appeared"
    return int((j & ~rose).sum()), int((j & rose).sum())


def junk_clock_model(P, st):
    """The model of the three clock steps on a junk-vote state: a third of
    each timer array due at NOW0."""
    G, L = JUNK_G, JUNK_L
    rng = np.random.default_rng(7800 + P)
    m = TimersModel(G, P, L, st)
    m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
    m.load(due_timers(rng, G * P, NOW0, 1 / 3), due_timers(rng, G * P, NOW0, 1 / 3))
    return m


def py_election_rounds(st, G, P, L, mask):
    """The rounds on the statement-level restatement (oracle/pyoracle.py):
    per group and round, StartElection of the candidates in peer order, every
    voter handles the candidates in peer order, every candidate folds its
    replies in voter order."""
    oracle_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    if oracle_dir not in sys.path:
        sys.path.insert(0, oracle_dir)
    import pyoracle as po
    rafts = po.from_soa(st, G, P, L)
    gf = np.zeros(G, np.int32)
    for g in range(G):
        for r in range(mask.shape[0]):
            cands = [p for p in range(P) if (int(mask[r, g]) >> p) & 1 and rafts[g * P + p].state != po.LEADER]
            args = {c: rafts[g * P + c].StartElection() for c in cands}
            reps = {}
            for v in range(P):
                for c in cands:
                    if c != v:
                        reps[(c, v)] = po.RequestVoteReply()
                        rafts[g * P + v].HandleRequestVote(args[c], reps[(c, v)])
            for c in cands:
                for v in range(P):
                    if c != v:
                        fl = rafts[g * P + c].tally(args[c], reps[(c, v)])
                        gf[g] |= G_ELECTED if fl & po.F_BECAME_LEADER else 0
                        gf[g] |= G_STEPPED_DOWN if fl & po.F_STEPPED_DOWN else 0
    return po.to_soa(rafts, st, G, P, L), gf
