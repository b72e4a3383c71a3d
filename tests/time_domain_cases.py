"""The top of the timers' time domain (include/mraft.h: now in [0, 2^30],
heartbeat < 2^30, election_hi <= 2^20, deadlines stay int32): every timer call
at now in {2^30 - 2, 2^30 - 1, 2^30} under the largest configuration, with
loaded deadlines drawn from {INT32_MIN, -1, 0, now - 1, now, now + 1,
INT32_MAX}. now + heartbeat reaches 2^31 - 1 exactly at now = 2^30. The run is
written once for any list of nodes (the model's ModelNode, an Engine) driven
in lockstep. Test infrastructure only."""
from __future__ import annotations

import numpy as np

from multiraft_amd._abi import LEADER, NOTE_RV_HANDLED, RV_ARGS
from timers_cases import leaders_in_place_state

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
TOP_CFG = dict(seed=0x70B, heartbeat=2**30 - 1, election_lo=2**20 - 1, election_hi=2**20)
TOP_NOWS = (2**30 - 2, 2**30 - 1, 2**30)
TOP_G, TOP_P, TOP_L = 33, 5, 16
OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


def top_state():
    return leaders_in_place_state(TOP_G, TOP_P, TOP_L, np.random.default_rng(8100), seed=8100)


def edge_values(now):
    return np.array([INT32_MIN, -1, 0, now - 1, now, now + 1, INT32_MAX], dtype=np.int64)


def edge_deadlines(rng, n, now):
    return rng.choice(edge_values(now), size=n).astype(np.int32)


def same_across(outs, ctx):
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b), ctx


def top_of_time_run(nodes, now, check, clock_nows=None):
    """enable, load, arm, ticker (full and cut), one note kind
    (MRAFT_NOTE_RV_HANDLED on a real RequestVote round) and three clock steps,
    all at `now` and each from freshly loaded edge deadlines — or, with
    clock_nows, the clock steps at those times with one load before the first.
    check(ctx, loaded) runs after every call (`loaded`: the last loaded pair)."""
    G, P = TOP_G, TOP_P
    gp = G * P
    rng = np.random.default_rng(8200 + now % 1000)
    loaded = [None, None]

    def load():
        loaded[:] = edge_deadlines(rng, gp, now), edge_deadlines(rng, gp, now)
        for n in nodes:
            n.timers_load(*loaded)

    for n in nodes:
        n.timers_enable(now=now, **TOP_CFG)
    check("enable", None)
    load()
    check("load", loaded)
    arm = np.concatenate([rng.integers(0, gp, size=gp // 4), [-1, gp]]).astype(np.int32)
    for n in nodes:
        n.timers_arm(arm, now)
    check("arm", loaded)
    for cap in (None, 3):
        load()
        same_across([n.ticker(now, cap, cap) for n in nodes], f"ticker cap {cap}")
        check(f"ticker cap {cap}", loaded)
    # one RequestVote round, the first non-leader of every group standing
    load()
    role = np.array(nodes[0].scalar_state()["state"]).reshape(G, P)
    cs = (np.arange(G) * P + (role != LEADER).argmax(axis=1)).astype(np.int32)
    reps = []
    for n in nodes:
        ra, serr = n.start_election(cs)
        assert not serr.any()
        q = np.tile(np.arange(P - 1), G)
        src = np.repeat(np.arange(G), P - 1)
        va = np.zeros(len(src), dtype=RV_ARGS)
        va["slot"] = (cs[src] // P) * P + np.where(q < cs[src] % P, q, q + 1)
        va["candidate_id"] = cs[src] % P
        for f in ("term", "last_log_index", "last_log_term"):
            va[f] = ra[f][src]
        rep, herr = n.handle_request_vote(va)
        assert not herr.any()
        n.timers_note(NOTE_RV_HANDLED, va, rep, herr, now)
        reps.append((rep, herr))
    same_across(reps, "RequestVote round")
    assert (reps[0][0]["vote_granted"] != 0).any()
    check("note", loaded)
    for k, t in enumerate(clock_nows or (now,) * 3):
        if k == 0 or not clock_nows:
            load()
        outs = [n.clock_step(t, bool(k % 2)) for n in nodes]
        same_across([[o[name] for name in OUTS] for o in outs], f"clock step {k} at {t}")
        check(f"clock step {k} at {t}", loaded)
