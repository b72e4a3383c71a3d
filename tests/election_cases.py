"""Exhaustive and directed cases of the election round
(multiraft_amd/csrc/mraft_elect_round.inc: the body of k_election_rounds and of
k_clock_round's election round) and their classification. Test infrastructure
only.

Three families, each returned as a case dict (G, P, L, st, mask[R, G] and the
family's own bookkeeping):

 exhaustive(P, B)   every group of P <= 3 replicas over currentTerm in
                    {B, B+1, B+2} x votedFor in {-1, 0..P-1, P (junk)} x state,
                    crossed with every round-0 timeout mask; a seeded last-entry
                    class per replica; the groups permuted, so a mask value does
                    not sit in a fixed lane segment.
 directed(P, B)     P in 4..8: per candidate position one group for every
                    reachable pair (lpos, spos) of the tally, one per voter class,
                    and the two-, three- and all-candidate scenarios.
 edge(P, G, L, R)   seeded groups over the log shapes the last-entry read can
                    meet (empty, snapshot-only, dummy > 0, last entry at physical
                    slot 0 and L-1, L = 1), at group counts around the segment,
                    wave and block edges.

classify() names each candidate's cell from the oracle's message-level records
(timers_model.deliver_round / tally_round: the RV_RESULT items in voter order)
and from nothing that restates the kernel."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from multiraft_amd._abi import CANDIDATE, FOLLOWER, LEADER
from multiraft_amd.engine import new_state
from oracle_lib import Oracle, assert_states_equal
from timers_cases import CFG, NOW0, due_timers
from timers_model import TimersModel, deliver_round, tally_round

L_SMALL = 4
BASES = (10, 2**31 - 64)
TERM_MAX = 2**31 - 1
DEAD = 99  # a term in the ring's dead slots: read by mistake, it would win every isLogUpToDate

# ---- assembling a state image ------------------------------------------------------


def place_log(L, head, terms):
    """The physical ring row of a log whose entries dummy..last carry `terms`."""
    row = np.full(L, DEAD, np.int32)
    for k, t in enumerate(terms):
        row[(head + k) % L] = t
    return row


def assemble(G, P, L, term, voted, role, votes, dummy, last, head, rows, dirty_seed=None):
    """A state image from per-replica arrays ([G*P], rows [G*P, L]). Leaders
    get matchIndex 0 and nextIndex in [dummy + 1, last + 1] (the tick's
    domain); dirty_seed: seeded nonzero persist bits instead of zeros."""
    st = new_state(G, P, L)
    gp = G * P
    st["current_term"][:] = np.asarray(term).reshape(gp)
    st["voted_for"][:] = np.asarray(voted).reshape(gp)
    st["state"][:] = np.asarray(role).reshape(gp)
    st["granted_votes"][:] = np.asarray(votes).reshape(gp)
    st["dummy_index"][:] = np.asarray(dummy).reshape(gp)
    st["last_index"][:] = np.asarray(last).reshape(gp)
    st["log_head"][:] = np.asarray(head).reshape(gp)
    st["log_term"][:] = np.asarray(rows, dtype=np.int32).reshape(gp * L)
    st["commit_index"][:] = st["dummy_index"]
    st["last_applied"][:] = st["dummy_index"]
    lead = st["state"] == LEADER
    span = (st["last_index"] - st["dummy_index"] + 1).astype(np.int64)
    s, j = np.arange(gp)[:, None], np.arange(P)[None, :]
    nxt = st["dummy_index"][:, None] + 1 + (s + j) % span[:, None]
    st["next_index"][:] = np.where(lead[:, None], nxt, 0).reshape(-1)
    if dirty_seed is not None:
        st["persist_dirty"][:] = np.random.default_rng(dirty_seed).integers(0, 4, gp)
    return st


def with_dirty(case, seed):
    """The case's state with seeded nonzero persist bits."""
    st = {k: v.copy() for k, v in case["st"].items()}
    st["persist_dirty"][:] = np.random.default_rng(seed).integers(0, 4, case["G"] * case["P"])
    return st


def take_groups(case, idx):
    """The case restricted to the groups `idx`."""
    G = case["G"]
    out = dict(case, G=len(idx), st={k: v.reshape(G, -1)[idx].reshape(-1).copy() for k, v in case["st"].items()},
               mask=np.ascontiguousarray(case["mask"][:, idx]))
    for k in ("cls", "tags"):
        if k in case:
            out[k] = case[k][idx]
    return out


def assert_images_equal(a, b, G, P, L, ctx):
    """Two state images after election calls, which write no log: every array
    equal as stored, dead ring slots included (assert_states_equal names the
    difference)."""
    if all(np.array_equal(v, b[k]) for k, v in a.items() if k in b):
        return
    assert_states_equal(a, b, G, P, L, ctx)
    raise AssertionError(f"{ctx}: log_term differs in dead ring slots")


def mask_bits(mask_row, P):
    """bool[G, P] of a mask row (bits at and above P dropped)."""
    return ((np.asarray(mask_row, np.int64)[:, None] >> np.arange(P)) & 1).astype(bool)


# ---- 1. exhaustive small groups ------------------------------------------------------
# last-entry classes, strictly ordered by isLogUpToDate: (lastTerm 5, last 2) < (5, 3) < (6, 1)
CLASS_LAST = np.array([2, 3, 1], np.int32)
CLASS_ROWS = np.array([[0, 5, 5, DEAD], [0, 4, 5, 5], [0, 6, DEAD, DEAD]], np.int32)
ROLES = np.array([LEADER, CANDIDATE, FOLLOWER], np.int32)
EXH_ROUNDS = 3


def exhaustive_size(P):
    return (9 * (P + 2)) ** P * 2 ** P


def exhaustive(P, B=10):
    """The exhaustive set of P-replica groups at term base B (built once per
    (P, B); callers leave it unchanged)."""
    return _exhaustive(P, B)


@functools.lru_cache(maxsize=None)
def _exhaustive(P, B):
    n1 = 9 * (P + 2)
    G = exhaustive_size(P)
    g = np.arange(G, dtype=np.int64)
    mask0, rest = g % 2 ** P, g // 2 ** P
    term, voted, role = (np.empty((G, P), np.int32) for _ in range(3))
    for p in range(P):
        code, rest = rest % n1, rest // n1
        term[:, p] = B + code % 3
        role[:, p] = ROLES[(code // 3) % 3]
        voted[:, p] = code // 9 - 1                  # -1, 0..P-1, P (junk)
    votes = (g[:, None] // 5 + g[:, None] + 2 * np.arange(P)[None, :]) % 3
    rng = np.random.default_rng(0xE1EC00 + P)
    cls = rng.integers(0, 3, (G, P))
    mask = np.concatenate([mask0[None, :], rng.integers(0, 2 ** P, (EXH_ROUNDS - 1, G))]).astype(np.uint8)
    perm = rng.permutation(G)
    term, voted, role, votes, cls = term[perm], voted[perm], role[perm], votes[perm], cls[perm]
    mask = np.ascontiguousarray(mask[:, perm])
    zero = np.zeros(G * P, np.int32)
    st = assemble(G, P, L_SMALL, term, voted, role, votes, zero, CLASS_LAST[cls], zero, CLASS_ROWS[cls.reshape(-1)])
    return dict(name=f"exhaustive P {P} B {B}", G=G, P=P, L=L_SMALL, B=B, st=st, mask=mask, cls=cls)


def exhaustive_subset(P, n, seed):
    """A seeded subset of n groups of exhaustive(P)."""
    case = exhaustive(P)
    idx = np.sort(np.random.default_rng(seed).choice(case["G"], n, replace=False))
    return dict(take_groups(case, idx), name=f"exhaustive P {P}, {n} groups")


CLOCK_SUBSET = 16384    # of exhaustive(3), for the clock step (the model loops over groups in Python)
PY_SUBSET = 4096        # of exhaustive(3), for the statement-level restatement


# ---- 2. the directed tally table -------------------------------------------------------
# log kinds of the table, relative to the candidate's (lastTerm 5, last 2): name -> (last, logical terms 0..last)
LOGS = {"cand": (2, [0, 5, 5]), "same": (2, [0, 3, 5]), "b_idx": (1, [0, 5]), "b_term": (3, [0, 4, 4, 4]),
        "a_idx": (3, [0, 4, 5, 5]), "a_term": (1, [0, 6])}
BEHIND = ("same", "b_idx", "b_term")

# voter classes: name -> (reply kind, role, term - args.Term, votedFor, log); votedFor "c" the candidate,
# "o" another replica, "v" the voter itself, "j" a junk value (P)
VOTERS = {
    "g_free": ("G", FOLLOWER, 0, -1, None),
    "g_again": ("G", FOLLOWER, 0, "c", None),
    "g_lower": ("G", FOLLOWER, -1, "o", None),
    "g_leader_lower": ("G", LEADER, -1, "v", None),
    "g_junk_lower": ("G", FOLLOWER, -1, "j", None),
    "e_voted_other": ("E", FOLLOWER, 0, "o", None),
    "e_log_term": ("E", FOLLOWER, -1, -1, "a_term"),
    "e_log_index": ("E", FOLLOWER, 0, -1, "a_idx"),
    "e_leader_equal": ("E", LEADER, 0, "v", None),
    "e_junk_equal": ("E", FOLLOWER, 0, "j", None),
    "h_follower": ("H", FOLLOWER, 1, -1, None),
    "h_leader": ("H", LEADER, 1, "v", None),
}
KINDS = {k: [n for n, v in VOTERS.items() if v[0] == k] for k in "GEH"}
DIRECTED_P = (4, 5, 6, 7, 8)
SCENARIO_P = (4, 5, 8)
SCENARIOS = ("equal", "lower_higher_term", "higher_higher_term", "all_equal", "all_staggered", "leader_bit_deposed",
             "leader_bit_alone", "high_bits", "three_equal") + tuple(f"three_{''.join(map(str, o))}"
                                                                     for o in itertools.permutations(range(3)))


def reachable_pairs(P, c):
    """Every (lpos, spos) a tally of candidate c can meet (voter peers, None:
    no such event), by counting: the P/2-th grant needs P/2 - 1 other voters
    before it that are not the first higher-term refusal."""
    others = [v for v in range(P) if v != c]
    need = P // 2
    out = []
    for lp in others + [None]:
        for sp in others + [None]:
            if lp is not None and lp == sp:
                continue
            if lp is not None:
                room = others.index(lp) - (1 if sp is not None and sp < lp else 0)
                if room < need - 1:
                    continue
            out.append((lp, sp))
    return out


def tally_layout(P, c, lpos, spos):
    """Reply kinds per voter peer for the cell (lpos, spos): grants (G) and
    equal-term refusals (E) mixed before the deciding event, a grant after it
    wherever a voter is left."""
    others = [v for v in range(P) if v != c]
    need = P // 2
    kind = {}
    if spos is not None:
        kind[spos] = "H"
    free = [v for v in others if v != spos]
    if lpos is not None:
        before, after = [v for v in free if v < lpos], [v for v in free if v > lpos]
        pick = before[0::2][:need - 1]
        pick += [v for v in before if v not in pick][:need - 1 - len(pick)]
        assert len(pick) == need - 1
        for v in before:
            kind[v] = "G" if v in pick else "E"
        kind[lpos] = "G"
        for i, v in enumerate(after):
            kind[v] = "G" if i % 2 == 0 else "E"
    else:
        after = [v for v in free if spos is not None and v > spos]
        before = [v for v in free if v not in after]
        pick = after[:1] if need - 1 >= 1 else []
        pick += before[0::2][:need - 1 - len(pick)]
        for v in free:
            kind[v] = "G" if v in pick else "E"
    return kind


class _Table:
    def __init__(self, P, B):
        self.P, self.B = P, B
        self.rows, self.masks, self.tags = [], [], []
        self.n = {k: 0 for k in "GEHcl"}

    def voter(self, name, c, v, at):
        P = self.P
        _, role, dt, vf, log = VOTERS[name]
        if log is None:
            log = BEHIND[self.n["l"] % 3]
            self.n["l"] += 1
        o = (c + 1) % P if (c + 1) % P != v or P < 3 else (c + 2) % P
        voted = {"c": c, "o": o, "v": v, "j": P}.get(vf, vf)
        return dict(term=at + dt, voted=voted, role=role, log=log, cls=name)

    def candidate(self, c, term, log="cand"):
        P, k = self.P, self.n["c"]
        self.n["c"] += 1
        voted = (-1, (c + 1) % P, c, P)[k % 4]
        return dict(term=term, voted=voted, role=(FOLLOWER, CANDIDATE)[k % 2], log=log, cls="candidate")

    def pick(self, kind):
        names = KINDS[kind]
        self.n[kind] += 1
        return names[(self.n[kind] - 1) % len(names)]

    def add(self, reps, mask, tag):
        assert len(reps) == self.P
        self.rows.append(reps)
        self.masks.append(mask)
        self.tags.append(tag)

    def case(self):
        P, B, G = self.P, self.B, len(self.rows)
        L = L_SMALL
        flat = [r for reps in self.rows for r in reps]
        gp = G * P
        votes = (np.arange(gp) // P + np.arange(gp)) % 3
        rows = np.stack([place_log(L, 0, LOGS[r["log"]][1]) for r in flat])
        st = assemble(G, P, L, [r["term"] for r in flat], [r["voted"] for r in flat], [r["role"] for r in flat], votes,
                      np.zeros(gp, np.int32), [LOGS[r["log"]][0] for r in flat], np.zeros(gp, np.int32), rows)
        rng = np.random.default_rng(0xD1EC00 + P)
        mask = np.concatenate([np.array(self.masks, np.int64)[None, :], rng.integers(0, 2 ** P, (2, G))]).astype(np.uint8)
        return dict(name=f"directed P {P} B {B}", G=G, P=P, L=L, B=B, st=st, mask=mask,
                    tags=np.array(self.tags, dtype=object), vcls=np.array([r["cls"] for r in flat], dtype=object))


def directed(P, B=10):
    """The directed table of P-replica groups at term base B (built once per
    (P, B); callers leave it unchanged)."""
    return _directed(P, B)


@functools.lru_cache(maxsize=None)
def _directed(P, B):
    t = _Table(P, B)
    at = B + 1
    for c in range(P):
        others = [v for v in range(P) if v != c]
        for lpos, spos in reachable_pairs(P, c):
            kind = tally_layout(P, c, lpos, spos)
            reps = [t.candidate(c, B) if v == c else t.voter(t.pick(kind[v]), c, v, at) for v in range(P)]
            t.add(reps, 1 << c, ("tally", c, lpos, spos))
        for name in VOTERS:                           # every voter class next to every candidate position
            reps = [t.candidate(c, B) if v == c else t.voter(name if v == others[0] else "g_free", c, v, at)
                    for v in range(P)]
            t.add(reps, 1 << c, ("voter", c, name))
    if P in SCENARIO_P:
        free = lambda v, term: dict(term=term, voted=-1, role=FOLLOWER, log=BEHIND[v % 3], cls="free")  # noqa: E731
        full = (1 << P) - 1
        for c1, c2 in itertools.combinations(range(P), 2):
            for tag, t1, t2 in (("equal", B, B), ("lower_higher_term", B + 1, B), ("higher_higher_term", B, B + 1)):
                reps = [t.candidate(v, t1 if v == c1 else t2) if v in (c1, c2) else free(v, B) for v in range(P)]
                t.add(reps, 1 << c1 | 1 << c2, (tag, c1, c2))
            # a Leader whose mask bit is set is no candidate: next to a candidate above its term, and alone
            ld = dict(term=B, voted=c1, role=LEADER, log="cand", cls="leader")
            reps = [ld if v == c1 else t.candidate(v, B + 1) if v == c2 else free(v, B) for v in range(P)]
            t.add(reps, 1 << c1 | 1 << c2, ("leader_bit_deposed", c1, c2))
            reps = [ld if v == c1 else free(v, B) for v in range(P)]
            t.add(reps, 1 << c1, ("leader_bit_alone", c1, c2))
            # mask bits at and above P (ignored): the equal-term pair again
            reps = [t.candidate(v, B) if v in (c1, c2) else free(v, B) for v in range(P)]
            t.add(reps, (1 << c1 | 1 << c2 | (0xFF << P)) & 0xFF, ("high_bits", c1, c2))
        for tri in itertools.combinations(range(P), 3):
            for tag, terms in [("three_equal", (B, B, B))] + [(f"three_{''.join(map(str, o))}", tuple(B + x for x in o))
                                                              for o in itertools.permutations(range(3))]:
                reps = [t.candidate(v, terms[tri.index(v)]) if v in tri else free(v, B) for v in range(P)]
                t.add(reps, sum(1 << v for v in tri), (tag,) + tri)
        t.add([t.candidate(v, B) for v in range(P)], full, ("all_equal",))
        t.add([t.candidate(v, B + v % 3) for v in range(P)], full, ("all_staggered",))
    return t.case()


# ---- 3. log and placement edges --------------------------------------------------------
EDGE_G = (1, 7, 8, 9, 31, 32, 33, 65)
EDGE_CASES = ([(P, G, L_SMALL, R) for i, G in enumerate(EDGE_G) for R, P in zip((0, 1, 2, 3), np.roll((3, 5, 8, 2, 4, 7, 1, 6), i))]
              + [(5, 65, L_SMALL, 65), (8, 33, L_SMALL, 65), (3, 9, L_SMALL, 65)]
              + [(1, 9, 1, 3), (2, 33, 1, 3), (2, 65, 1, 65)])
EDGE_CASES = [tuple(int(x) for x in c) for c in EDGE_CASES]


def edge_logs(L):
    """name -> (dummy, logical terms dummy..last, head or None: any)."""
    kinds = {"empty": (0, [0], None), "snap_term5": (7, [5], None), "snap_term6": (7, [6], None),
             "snap_far": (9, [5], None)}
    if L >= 4:
        kinds.update({"dummy_entries": (7, [3, 5, 5], None), "last_at_slot0": (6, [2, 5, 6], L - 2),
                      "last_at_slotL1": (6, [2, 5, 5], L - 3), "full": (0, [0] + [5] * (L - 1), None)})
    return kinds


@functools.lru_cache(maxsize=None)
def edge(P, G, L, R):
    rng = np.random.default_rng(0xED6E00 + 1000 * P + 10 * G + L + 7 * R)
    kinds = edge_logs(L)
    names = list(kinds)
    gp = G * P
    kidx = rng.integers(0, len(names), gp)
    head = rng.integers(0, L, gp)
    dummy, last, rows = np.zeros(gp, np.int32), np.zeros(gp, np.int32), np.zeros((gp, L), np.int32)
    for s in range(gp):
        d, terms, h = kinds[names[kidx[s]]]
        head[s] = head[s] if h is None else h
        dummy[s], last[s] = d, d + len(terms) - 1
        rows[s] = place_log(L, int(head[s]), terms)
    role = np.where(rng.random(gp) < 0.2, LEADER, np.where(rng.random(gp) < 0.5, CANDIDATE, FOLLOWER))
    st = assemble(G, P, L, 10 + rng.integers(0, 3, gp), rng.integers(-1, P + 1, gp), role, rng.integers(0, 3, gp),
                  dummy, last, head, rows)
    bits = rng.random((max(R, 1), G, 8)) < 0.4
    bits[:, :, P:] &= rng.random((max(R, 1), G, 1)) < 0.25          # bits at and above P, now and then
    mask = (bits << np.arange(8)).sum(axis=2).astype(np.uint8)[:R]
    return dict(name=f"edge P {P} G {G} L {L} R {R}", G=G, P=P, L=L, B=10, st=st, mask=mask.reshape(R, G),
                kinds=np.array(names, dtype=object)[kidx])


def last_entry_slot(st, L):
    """Physical ring slot of every replica's last entry."""
    return (st["log_head"].astype(np.int64) + st["last_index"] - st["dummy_index"]) % L


# ---- classification from the message-level records ----------------------------------------
def candidates_of(st, mask_row, P):
    """Slots that run StartElection in a round: mask bit set and not Leader."""
    bits = mask_bits(mask_row, P).reshape(-1)
    return np.nonzero(bits & (st["state"] != LEADER))[0].astype(np.int32)


def classify(o, cslots):
    """Run one message-level round on the oracle `o` for the candidates
    `cslots` and name each candidate's tally cell from the RV_RESULT items, in
    voter order: lpos, the voter peer of the first item at which the cumulative
    grants exceed P/2 - 1 (-1: none); spos, the voter peer of the first refusal
    with reply_term > args_term (-1: none); guard, whether the closure's guard
    (raft_election.go:29) held at the first item (the oracle's state between
    the deliveries and the tally). Also the items [n, P-1], the per-item tally
    flags, and each candidate's number of grants."""
    G, P = o.G, o.P
    items, seg, _ = deliver_round(o, G, P, cslots)
    n = len(cslots)
    if items is None:
        return dict(slot=cslots, lpos=np.full(n, -1), spos=np.full(n, -1), guard=np.ones(n, bool), items=None,
                    grants=np.zeros(n, np.int64))
    it = items.reshape(n, P - 1)
    guard = (o.st["current_term"][cslots] == it["args_term"][:, 0]) & (o.st["state"][cslots] == CANDIDATE)
    gr = it["vote_granted"] != 0
    hit_l = gr & (np.cumsum(gr, axis=1) == P // 2)                # cumulative grants first exceed P/2 - 1
    hit_s = ~gr & (it["reply_term"] > it["args_term"])
    rows = np.arange(n)
    lpos = np.where(hit_l.any(axis=1), it["peer"][rows, hit_l.argmax(axis=1)], -1)
    spos = np.where(hit_s.any(axis=1), it["peer"][rows, hit_s.argmax(axis=1)], -1)
    _, _, fl = tally_round(o, G, P, items, seg)
    return dict(slot=cslots, lpos=lpos, spos=spos, guard=guard, items=it, flags=fl.reshape(n, P - 1),
                grants=gr.sum(axis=1))


def classify_case(case, r=0):
    """classify() of round r of a case, on a fresh oracle advanced by
    election_rounds to that round. Returns (records, the state before the
    round, the oracle after it)."""
    o = Oracle(case["G"], case["P"], case["L"], case["st"])
    if r:
        o.election_rounds(case["mask"][:r])
    before = o.store_state()
    return classify(o, candidates_of(before, case["mask"][r], case["P"])), before, o


def max_term_after(case, launches=2):
    """The highest term the oracle reaches over `launches` launches of the
    case's mask (the domain check of the high term base)."""
    o = Oracle(case["G"], case["P"], case["L"], case["st"])
    for _ in range(launches):
        o.election_rounds(case["mask"])
    return int(o.st["current_term"].max())


# ---- the clock step on these states ---------------------------------------------------------
def clock_timers(case, seed):
    """(election_due, heartbeat_due) with the election timers due at NOW0
    exactly where round 0's mask has a bit below P (a Leader's among them: its
    timer is reset and it is no candidate), others falling due at NOW0 + 1, and
    a third of the heartbeat timers due."""
    G, P = case["G"], case["P"]
    rng = np.random.default_rng(seed)
    n = G * P
    due = mask_bits(case["mask"][0], P).reshape(-1)
    ed = np.where(due, NOW0 - rng.integers(0, 3, n), NOW0 + rng.integers(1, 3, n)).astype(np.int32)
    return ed, due_timers(rng, n, NOW0, 1 / 3)


def clock_model(case, seed=0xC10C):
    m = TimersModel(case["G"], case["P"], case["L"], case["st"])
    m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
    m.load(*clock_timers(case, seed))
    return m


CLOCK_STEPS = 2
CLOCK_OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


# ---- the message-level round on two nodes in lockstep -----------------------------------------
class Lockstep:
    """An Engine and an Oracle behind the three message-level methods: every
    call runs on both, and every reply, flag and error array and the whole
    state after the call must be equal."""

    def __init__(self, engine, oracle, assert_states_equal, ctx):
        self.e, self.o, self.eq, self.ctx = engine, oracle, assert_states_equal, ctx
        self.G, self.P, self.L = oracle.G, oracle.P, oracle.L
        self.calls = 0

    def _both(self, name, *a):
        got, want = getattr(self.e, name)(*a), getattr(self.o, name)(*a)
        ctx = f"{self.ctx}: {name} (call {self.calls})"
        self.calls += 1
        for k, (x, y) in enumerate(zip(got, want)):
            assert x.dtype == y.dtype and np.array_equal(x, y), (ctx, "output", k)
        self.eq(self.e.store_state(), self.o.state(), self.G, self.P, self.L, ctx)
        return want

    def start_election(self, slots):
        return self._both("start_election", slots)

    def handle_request_vote(self, args):
        return self._both("handle_request_vote", args)

    def process_vote_replies(self, items, seg):
        return self._both("process_vote_replies", items, seg)
