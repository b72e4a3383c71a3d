"""State builders, mask classes and schedules of the reachability tests
(mraft_set_reachable; tests/test_reach_cases.py on the CPU,
tests/test_reach_gpu.py on the engine). Test infrastructure only.

Everything a GPU test runs is built here from seeds, and what the built cases
contain is counted from the model's records (tests/reach_model.py), as the
other *_cases.py files do."""
from __future__ import annotations

import functools

import numpy as np

import election_cases as ec
from multiraft_amd import synth_seed, synth_tick_state
from multiraft_amd._abi import LEADER
from multiraft_amd.engine import new_state
from oracle_lib import Oracle
from random_states import random_tick_state
from reach_model import ReachModel, connected, full_mask, masked_tick
from timers_cases import CFG, CLOCK_CASES, NOW0, clock_case

# ---- the tick's mask classes ---------------------------------------------------------
TICK_CLASSES = ("full", "leader_clear", "follower_clear", "leader_plus_one", "majority", "one_short", "high_bits")


def followers(P, lp):
    return [q for q in range(P) if q != lp]


def tick_mask(cls, P, lp, k):
    """The mask of class `cls` for a group of P replicas led by peer lp; k picks
    among the followers (any integer)."""
    full = (1 << P) - 1
    lp = lp if 0 <= lp < P else 0
    fs = followers(P, lp)
    fs = fs[k % len(fs):] + fs[:k % len(fs)] if fs else fs

    def led(n):  # the leader and its n first followers
        return (1 << lp) | sum(1 << f for f in fs[:n])

    if cls == "full":
        return full
    if cls == "leader_clear":
        return full & ~(1 << lp)
    if cls == "follower_clear":
        return full & ~(1 << fs[0]) if fs else full
    if cls == "leader_plus_one":
        return led(1)
    if cls == "majority":          # P/2 + 1 connected: exactly a majority
        return led(P // 2)
    if cls == "one_short":         # P/2 connected
        return led(P // 2 - 1) if P >= 2 else 0
    if cls == "high_bits":         # bits at and above P are ignored
        return (led(P // 2) | (0xFF & ~full)) if P < 8 else led(P // 2)
    raise KeyError(cls)


def tick_masks(P, lp, seed):
    """One mask per group, the classes dealt round-robin from a seeded offset
    (so neighbouring groups, shards and list segments carry different masks)."""
    G = len(lp)
    cls = [TICK_CLASSES[(g + seed) % len(TICK_CLASSES)] for g in range(G)]
    m = np.array([tick_mask(c, P, int(lp[g]), g // len(TICK_CLASSES) + seed) for g, c in enumerate(cls)], np.uint8)
    return m, cls


TICK_P = (2, 3, 4, 5, 6, 7, 8)
TICK_G = (1, 7, 8, 9, 33, 65)
TICK_L = 64


@functools.lru_cache(maxsize=None)
def tick_case(P, G, seed, kind="fuzz"):
    """(st, lp, reach, classes). kind: "fuzz" (random_tick_state: stale and
    higher-term followers, conflicts, a3 panics, bad states), "snap" (its
    snapshot-heavy variant), "synth" (the bench generator's steady state)."""
    L = TICK_L
    rng = np.random.default_rng(0x5EAC00 + 131 * P + 7 * G + seed)
    if kind == "synth":
        st, lp, _ = synth_tick_state(G, P, L, seed=synth_seed(3) + seed)
    else:
        st, lp = random_tick_state(rng, G, P, L, monotone=bool(seed % 2), snap=(kind == "snap"))
    reach, cls = tick_masks(P, lp, seed)
    return st, np.asarray(lp, np.int32), reach, cls


def chunk_edge_case():
    """L = 1,024, P = 3, leader at peer 0 with 900 entries of one term. In each
    group one follower is delivered and merges 700 entries from Index 201, across
    the 256-entry chunk edges, while the other, cut off, sits at nextIndex 5 and
    would have started the pass there. The second follower's log differs from
    the leader's above Index 4, so a pass that started low would compare it."""
    G, P, L = 4, 3, 1024
    st = new_state(G, P, L)
    lt = st["log_term"].reshape(G * P, L)
    lp = np.zeros(G, np.int32)
    reach = np.zeros(G, np.uint8)
    for g in range(G):
        ld = g * P
        head = (37 * g) % L                                # rotated rings too
        for r in range(P):
            st["log_head"][ld + r] = (head + 5 * r) % L
        last = 900 + g
        lt[ld, (st["log_head"][ld] + np.arange(last + 1)) % L] = np.r_[0, np.full(last, 3)]
        st["last_index"][ld] = last
        st["current_term"][ld:ld + P] = 3
        st["state"][ld] = LEADER
        st["state"][ld + 1:ld + P] = 3
        st["commit_index"][ld] = 100
        near, far = (1, 2) if g % 2 == 0 else (2, 1)       # the delivered follower, the one cut off
        nl = 200 + 17 * g
        lt[ld + near, (st["log_head"][ld + near] + np.arange(nl + 1)) % L] = np.r_[0, np.full(nl, 3)]
        st["last_index"][ld + near] = nl
        st["next_index"][ld * P + near] = nl + 1
        st["match_index"][ld * P + near] = nl
        lt[ld + far, (st["log_head"][ld + far] + np.arange(40)) % L] = np.r_[0, np.full(4, 3), np.full(35, 2)]
        st["last_index"][ld + far] = 39
        st["next_index"][ld * P + far] = 5
        st["match_index"][ld * P + far] = 4
        reach[g] = (1 << 0) | (1 << near)
    return G, P, L, st, lp, reach


def would_reply(o_state, G, P, L, lp):
    """What every follower would reply on a perfect network: the record of a
    full-mask model tick on a copy. Classes per follower: merge, heartbeat,
    conflict (no success, term not higher), stale (reply term higher), snapshot,
    log_full."""
    rec = {}
    o = Oracle(G, P, L, o_state)
    masked_tick(o, lp, full_mask(G, P), rec)
    return rec


def undelivered_classes(st, G, P, L, lp, reach):
    """Counts, over the followers the mask cuts off from a running leader, of the
    reply class each would have had."""
    rec = would_reply(st, G, P, L, lp)
    conn = connected(reach, G, P)
    lpc = np.clip(lp, 0, P - 1)
    cut = rec["delivered"] & ~(conn & conn[np.arange(G), lpc][:, None])
    n = rec["n_entries"]
    ok = rec["ae"] & rec["reply_success"]
    return {
        "merge": int((cut & ok & (n > 0)).sum()),
        "heartbeat": int((cut & ok & (n == 0)).sum()),
        "conflict": int((cut & rec["ae"] & ~rec["log_full"] & ~rec["reply_success"] & ~rec["reply_term_higher"]).sum()),
        "stale": int((cut & rec["reply_term_higher"]).sum()),
        "snapshot": int((cut & rec["snap"]).sum()),
        "log_full": int((cut & rec["log_full"]).sum()),
    }


# ---- the election round's masks ---------------------------------------------------------
ROUND_CLASSES = ("full", "cand_cut", "majority", "one_short")


def round_mask_for(cls, P, c, k=0):
    """Mask of a round class around candidate c: "voter_cut" cuts the k-th
    other replica, "majority" / "one_short" connect c and P/2 / P/2 - 1 others."""
    full = (1 << P) - 1
    others = [q for q in range(P) if q != c]

    def around(n):
        return (1 << c) | sum(1 << q for q in others[:n])

    if cls == "full":
        return full
    if cls == "cand_cut":
        return full & ~(1 << c)
    if cls == "voter_cut":
        return full & ~(1 << others[k % len(others)])
    if cls == "majority":
        return around(P // 2)
    if cls == "one_short":
        return around(P // 2 - 1)
    raise KeyError(cls)


def directed_round_masks(case, cls, k=0):
    """Per group of a directed case (election_cases.directed): the class's mask
    around the group's lowest round-0 candidate."""
    P = case["P"]
    m0 = case["mask"][0]
    out = np.zeros(case["G"], np.uint8)
    for g in range(case["G"]):
        bits = int(m0[g]) & ((1 << P) - 1)
        c = (bits & -bits).bit_length() - 1 if bits else 0
        out[g] = round_mask_for(cls, P, c, k)
    return out


P3_SAMPLE = 32768   # groups of exhaustive(3) per mask (8 masks): the CPU model takes about 1 s per mask


def p3_sample(mask):
    return ec.exhaustive_subset(3, P3_SAMPLE, seed=0x3EAC + mask)


# ---- the clock step --------------------------------------------------------------------------
CLOCK_STEPS = 6
CLOCK_MASK_EVERY = 2


def clock_masks(P, G, send_all, epoch):
    """Seeded masks of one clock case for the steps of `epoch`: a third of the
    groups fully connected, the others any byte."""
    rng = np.random.default_rng(0xC1AC + 1000 * epoch + 31 * P + 7 * G + int(send_all))
    m = rng.integers(0, 256, G).astype(np.uint8)
    m[rng.random(G) < 1 / 3] = (1 << P) - 1
    return m


def clock_model(P, G, send_all):
    L, st, ed, hd = clock_case(P, G, send_all)
    m = ReachModel(G, P, L, st)
    m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
    m.load(ed, hd)
    return L, st, ed, hd, m


# ---- the reference's connect / disconnect schedules (src/raft/test_test.go) ----------------------
# One phase lasts 2 * election_hi ticks. A phase's mask is a function of the
# group's leader when the phase begins (L: that leader; M: the leader remembered
# from the phase marked "mark").
# (With the timeout range [10, 20) the model alone showed one 2-of-3 partition
# whose two candidates split their votes past 2 * election_hi ticks: Raft's
# liveness is probabilistic. The range is [10, 30), three heartbeats wide per
# step as the reference's 150-300 ms over 50 ms; chosen on the model, before any
# engine run.)
SCEN_CFG = dict(seed=7, heartbeat=3, lo=10, hi=30)
SCEN_PHASE = 2 * SCEN_CFG["hi"]
SCEN_L = 128


def _full(P, L, M):
    return (1 << P) - 1


def _without(*offs):
    return lambda P, L, M: ((1 << P) - 1) & ~sum(1 << ((L + o) % P) for o in offs)


def _without_marked(*offs):
    return lambda P, L, M: ((1 << P) - 1) & ~sum(1 << ((M + o) % P) for o in offs)


SCENARIOS = {
    # TestReElection2A: leader1 out; back; leader2 and leader2+1 out (no quorum); leader2+1 back; all back
    "ReElection2A": (3, [(_full, False), (_without(0), False), (_full, False), (_without(0, 1), True),
                         (_without_marked(0), False), (_full, False)]),
    # TestFailAgree2B: follower leader+1 out for two phases (agreement goes on), then back
    "FailAgree2B": (3, [(_full, False), (_without(1), True), (_without_marked(1), False), (_full, False)]),
    # TestFailNoAgree2B: three of five followers out (Start at the leader: no commit), then back
    "FailNoAgree2B": (5, [(_full, False), (_without(1, 2, 3), False), (_full, False), (_full, False)]),
    # TestRejoin2B: leader1 out (it keeps appending), leader2 out and leader1 back, all back
    "Rejoin2B": (3, [(_full, False), (_without(0), False), (_without(0), False), (_full, False)]),
}


def scenario_groups(P, G):
    """Scenario name per group for a run with P replicas per group."""
    names = [n for n, (p, _) in SCENARIOS.items() if p == P]
    return [names[g % len(names)] for g in range(G)]


def visible_leader(state, term, conn_row):
    """The connected Leader with the highest term (lowest peer on a tie), or the
    highest-term Leader at all when none is connected, or 0."""
    best, key = 0, (-1, -1)
    for p in range(len(state)):
        if state[p] == LEADER:
            k = (int(bool(conn_row[p])), int(term[p]))
            if k > key:
                best, key = p, k
    return best


# ---- hand-derived known answers ----------------------------------------------------------------
# Small states written out by hand; `expect` maps a state array to {index: value}
# after the call, worked out from the cited Go lines, `same` lists replicas whose
# every scalar must be untouched.
def _ka_tick_state(P):
    """Leader 0 at term 2 with log terms [0, 1, 2, 2] (Indexes 0..3), commitIndex 1;
    every follower holds [0, 1], term 2, commitIndex 0, nextIndex 2, matchIndex 1."""
    G, L = 1, 8
    st = new_state(G, P, L)
    lt = st["log_term"].reshape(P, L)
    lt[0, :4] = [0, 1, 2, 2]
    lt[1:, :2] = [0, 1]
    st["last_index"][:] = [3] + [1] * (P - 1)
    st["current_term"][:] = 2
    st["state"][:] = [LEADER] + [3] * (P - 1)
    st["commit_index"][0] = 1
    st["last_applied"][0] = 1
    st["next_index"][:P] = 2
    st["match_index"][:P] = 1
    return G, P, L, st


def known_answers():
    ka = []
    A, C, FC = 1, 2, 32   # MRAFT_G_ACTIVE, _COMMITTED, _FOLLOWER_COMMIT
    # 1. mask 0b011: follower 1 appends Indexes 2, 3 (raft_append_entry.go:149-155) and
    # follows leaderCommit 1 (:157-160); its reply sets matchIndex[1] = 3, nextIndex[1] = 4
    # (:76-77); matchIndex {leader 3, 3, 1}: the majority holds 3 and term(3) = currentTerm,
    # so commitIndex = 3 (:89-105) on 2 of 3. Follower 2 hears nothing.
    G, P, L, st = _ka_tick_state(3)
    ka.append(dict(name="tick 0b011", kind="tick", G=G, P=P, L=L, st=st, lp=[0], reach=[0b011], flags=[A | C | FC],
                   expect={"last_index": {1: 3}, "commit_index": {0: 3, 1: 1}, "match_index": {1: 3, 2: 1},
                           "next_index": {1: 4, 2: 2}, "persist_dirty": {0: 0, 1: 1, 2: 0}}, same=[2]))
    # 2. mask 0b001: nothing is delivered
    G, P, L, st = _ka_tick_state(3)
    ka.append(dict(name="tick 0b001", kind="tick", G=G, P=P, L=L, st=st, lp=[0], reach=[0b001], flags=[A],
                   expect={}, same=[0, 1, 2]))
    # 3. P = 5, leader and follower 1 connected: matchIndex {3, 3, 1, 1, 1}, the majority
    # holds 1 = commitIndex: no commit
    G, P, L, st = _ka_tick_state(5)
    ka.append(dict(name="tick P 5 two connected", kind="tick", G=G, P=P, L=L, st=st, lp=[0], reach=[0b00011],
                   flags=[A | FC], expect={"last_index": {1: 3}, "commit_index": {0: 1, 1: 1}, "match_index": {1: 3}},
                   same=[2, 3, 4]))
    # 4. the leader's own bit clear, both followers connected: it delivers nothing
    G, P, L, st = _ka_tick_state(3)
    ka.append(dict(name="tick leader cut off", kind="tick", G=G, P=P, L=L, st=st, lp=[0], reach=[0b110], flags=[A],
                   expect={}, same=[0, 1, 2]))

    def followers_state(P):
        G, L = 1, 4
        st = new_state(G, P, L)
        st["current_term"][:] = 1
        return G, P, L, st

    E = 128  # MRAFT_G_ELECTED
    # 5. candidate 0, mask 0b011: StartElection (raft_election.go:4-15) term 2, votes 1; voter 1
    # adopts term 2 and grants (:63-74); 2 > 3/2: Leader (:32-38). Replica 2 hears nothing.
    G, P, L, st = followers_state(3)
    ka.append(dict(name="round 0b011", kind="round", G=G, P=P, L=L, st=st, cand=[0b001], reach=[0b011], flags=[E],
                   expect={"current_term": {0: 2, 1: 2, 2: 1}, "state": {0: LEADER, 1: 3, 2: 3},
                           "granted_votes": {0: 2}, "voted_for": {0: 0, 1: 0, 2: -1},
                           "persist_dirty": {0: 1, 1: 1, 2: 0}}, same=[2]))
    # 6. the same candidate cut off: Candidate, its own vote, term + 1
    G, P, L, st = followers_state(3)
    ka.append(dict(name="round candidate cut off", kind="round", G=G, P=P, L=L, st=st, cand=[0b001], reach=[0b110],
                   flags=[0], expect={"current_term": {0: 2}, "state": {0: 2}, "granted_votes": {0: 1},
                                      "voted_for": {0: 0}, "persist_dirty": {0: 1, 1: 0, 2: 0}}, same=[1, 2]))
    # 7. candidates 0 and 1, replica 1 cut off: 0 is elected on voter 2's grant, 1 stays Candidate
    G, P, L, st = followers_state(3)
    ka.append(dict(name="round two candidates, one cut off", kind="round", G=G, P=P, L=L, st=st, cand=[0b011],
                   reach=[0b101], flags=[E],
                   expect={"current_term": {0: 2, 1: 2, 2: 2}, "state": {0: LEADER, 1: 2, 2: 3},
                           "granted_votes": {0: 2, 1: 1}, "voted_for": {0: 0, 1: 1, 2: 0}}, same=[]))
    # 8. a stale Leader (replica 0, term 1) beside the Leader of term 2 (replica 1): cut off it
    # stays Leader; rejoined, the next heartbeat's higher term makes it a follower
    # (raft_append_entry.go:116-120)
    G, L, P = 1, 4, 3
    st = new_state(G, P, L)
    st["current_term"][:] = [1, 2, 2]
    st["state"][:] = [LEADER, LEADER, 3]
    st["next_index"][P:2 * P] = 1
    ka.append(dict(name="stale leader cut off", kind="tick", G=G, P=P, L=L, st=st, lp=[1], reach=[0b110], flags=[A],
                   expect={"current_term": {0: 1}, "state": {0: LEADER}}, same=[0]))
    ka.append(dict(name="stale leader rejoins", kind="tick", G=G, P=P, L=L, st=st, lp=[1], reach=[0b111], flags=[A],
                   expect={"current_term": {0: 2}, "state": {0: 3}, "voted_for": {0: -1}}, same=[]))
    return ka


SCALARS = ("current_term", "voted_for", "state", "commit_index", "last_applied", "dummy_index", "last_index",
           "granted_votes", "persist_dirty", "log_head", "has_snapshot")


def check_known_answer(ka, flags, after):
    """`flags` and the state `after` the call against the hand-derived answer."""
    assert list(flags) == ka["flags"], (ka["name"], list(flags))
    for arr, want in ka["expect"].items():
        for i, v in want.items():
            assert after[arr][i] == v, (ka["name"], arr, i, int(after[arr][i]), v)
    for r in ka["same"]:
        for arr in SCALARS:
            assert after[arr][r] == ka["st"][arr][r], (ka["name"], "replica untouched", r, arr)
        L = ka["L"]
        assert np.array_equal(after["log_term"][r * L:(r + 1) * L], ka["st"]["log_term"][r * L:(r + 1) * L])
