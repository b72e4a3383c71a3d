"""CPU proofs about the election-round cases (tests/election_cases.py, run on
the GPU by tests/test_election_cases_gpu.py): the exhaustive sets are the whole
product and reach every lane position and every ordered pair of last-entry
classes; the directed table holds every reachable (lpos, spos) cell of the
tally, every voter class and every multi-candidate scenario for every (P, c),
classified from the oracle's message-level records; the edge set holds every
log shape as a candidate's and as a voter's; the high term base stays below
2^31 - 1; Oracle.election_rounds equals the oracle's own message-level
composition on every set (TimersModel._round asserts it), and the
statement-level restatement (oracle/pyoracle.py) equals the C oracle. Every
proof names the cells it misses."""
import itertools

import numpy as np
import pytest

import election_cases as ec
from junk_vote_cases import py_election_rounds
from oracle_lib import Oracle, assert_states_equal
from timers_cases import NOW0
from timers_model import TimersModel

from multiraft_amd._abi import CANDIDATE, FOLLOWER, LEADER

CLASS_NAMES = ("(5,2)", "(5,3)", "(6,1)")


# ---- 1. the exhaustive sets ------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3])
def test_exhaustive_is_the_whole_product(P):
    c = ec.exhaustive(P)
    G, st = c["G"], c["st"]
    assert G == {1: 54, 2: 5184, 3: 729000}[P] == ec.exhaustive_size(P)
    term = st["current_term"].reshape(G, P).astype(np.int64) - c["B"]
    voted = st["voted_for"].reshape(G, P).astype(np.int64) + 1
    role = st["state"].reshape(G, P).astype(np.int64) - 1
    assert term.min() == 0 and term.max() == 2 and voted.min() == 0 and voted.max() == P + 1
    assert set(np.unique(role)) == {0, 1, 2}
    code = c["mask"][0].astype(np.int64)
    for p in range(P):
        code = (code * 3 + term[:, p]) * 3 + role[:, p]
        code = code * (P + 2) + voted[:, p]
    assert len(np.unique(code)) == G, "a group of the product occurs twice, so another is missing"
    assert set(np.unique(st["granted_votes"])) == {0, 1, 2}
    lead = st["state"] == LEADER
    nxt = st["next_index"].reshape(G * P, P)
    assert (nxt[lead] >= 1).all() and (nxt[lead] <= st["last_index"][lead][:, None] + 1).all()
    assert not st["match_index"].any()


@pytest.mark.parametrize("P", [1, 2, 3])
def test_exhaustive_masks_reach_every_lane_position(P):
    c = ec.exhaustive(P)
    g = np.arange(c["G"])
    missing = []
    for r in range(ec.EXH_ROUNDS):
        for m in range(2 ** P):
            at = g[c["mask"][r] == m]
            missing += [f"round {r} mask {m}: segment {s}" for s in set(range(8)) - set(at % 8)]
            missing += [f"round {r} mask {m}: wave {w}" for w in set(range(4)) - set((at // 8) % 4)]
    assert not missing, missing
    if P > 1:  # the later rounds' masks do not follow round 0's
        assert len({tuple(x) for x in c["mask"].T}) == (2 ** P) ** ec.EXH_ROUNDS


@pytest.mark.parametrize("P", [2, 3])
def test_exhaustive_log_classes_meet_at_every_position(P):
    c = ec.exhaustive(P)
    G, cls = c["G"], c["cls"]
    cand = ec.mask_bits(c["mask"][0], P) & (c["st"]["state"].reshape(G, P) != LEADER)
    missing = []
    for cp in range(P):
        for vp in range(P):
            if cp == vp:
                continue
            have = set(zip(cls[cand[:, cp], cp], cls[cand[:, cp], vp]))
            missing += [f"candidate {cp} class {CLASS_NAMES[a]} / voter {vp} class {CLASS_NAMES[b]}"
                        for a in range(3) for b in range(3) if (a, b) not in have]
    assert not missing, missing
    # the classes are strictly ordered by isLogUpToDate (raft_log.go:99-104)
    lt = [int(ec.CLASS_ROWS[k][ec.CLASS_LAST[k]]) for k in range(3)]
    key = [(lt[k], int(ec.CLASS_LAST[k])) for k in range(3)]
    assert key[0] < key[1] < key[2]


# ---- 2. the directed table ----------------------------------------------------------------
@pytest.fixture(scope="module", params=ec.DIRECTED_P)
def table(request):
    case = ec.directed(request.param)
    rec, before, o = ec.classify_case(case)
    return case, rec, before, o


def brute_pairs(P, c):
    """Every (lpos, spos) over all 3^(P-1) ways to answer candidate c with a
    grant, an equal-term refusal or a higher-term refusal per voter (-1: no
    such event): the table's claim of what is reachable, counted here by the
    definition alone."""
    others = [v for v in range(P) if v != c]
    out = set()
    for kinds in itertools.product("GEH", repeat=P - 1):
        grants, lp, sp = 0, -1, -1
        for v, k in zip(others, kinds):
            grants += k == "G"
            if k == "G" and grants == P // 2:
                lp = v
            if k == "H" and sp < 0:
                sp = v
        out.add((lp, sp))
    return out


def _by_group(rec, P):
    return {int(s) // P: i for i, s in enumerate(rec["slot"])}     # single-candidate groups only


def test_directed_table_holds_every_tally_cell(table):
    case, rec, before, o = table
    P, tags = case["P"], case["tags"]
    row = _by_group(rec, P)
    have, wrong, missing = set(), [], []
    for g, tag in enumerate(tags):
        if tag[0] != "tally":
            continue
        _, c, lpos, spos = tag
        i = row[g]
        assert rec["slot"][i] == g * P + c and rec["guard"][i], tag
        got = (int(rec["lpos"][i]), int(rec["spos"][i]))
        want = (-1 if lpos is None else lpos, -1 if spos is None else spos)
        if got != want:
            wrong.append((tag, got))
        have.add((c,) + got)
        # a grant lies after the deciding event wherever a voter is left there, and the oracle did not count it
        it = rec["items"][i]
        events = [x for x in got if x >= 0]
        if events and [v for v in range(P) if v != c and v > min(events) and v != got[1]]:
            after = it["peer"] > min(events)
            assert (it["vote_granted"][after] != 0).any(), ("no grant after the deciding event", tag)
            assert o.st["granted_votes"][g * P + c] - 1 < rec["grants"][i], tag
    for c in range(P):
        missing += [f"P {P} c {c}: lpos {lp} spos {sp}" for lp, sp in sorted(brute_pairs(P, c)) if (c, lp, sp) not in have]
    assert not wrong, wrong
    assert not missing, missing
    for c in range(P):  # and the builder's own count of the reachable cells is that set
        claimed = {(-1 if lp is None else lp, -1 if sp is None else sp) for lp, sp in ec.reachable_pairs(P, c)}
        assert claimed == brute_pairs(P, c), (c, sorted(claimed ^ brute_pairs(P, c)))
    # the outcome the records imply is the oracle's: Leader when lpos comes first, Follower when spos does
    for g, tag in enumerate(tags):
        if tag[0] != "tally":
            continue
        i, s = row[g], g * P + tag[1]
        lp, sp = int(rec["lpos"][i]), int(rec["spos"][i])
        first_l = lp >= 0 and (sp < 0 or lp < sp)
        first_s = sp >= 0 and (lp < 0 or sp < lp)
        assert o.st["state"][s] == (LEADER if first_l else FOLLOWER if first_s else CANDIDATE), tag


def test_directed_table_holds_every_voter_class(table):
    case, rec, before, o = table
    P, tags = case["P"], case["tags"]
    row = _by_group(rec, P)
    have, missing = set(), []
    for g, tag in enumerate(tags):
        if tag[0] != "voter":
            continue
        _, c, name = tag
        v = [x for x in range(P) if x != c][0]
        assert case["vcls"][g * P + v] == name
        it = rec["items"][row[g]]
        item = it[it["peer"] == v][0]
        kind = ("G" if item["vote_granted"] else "H" if item["reply_term"] > item["args_term"] else "E")
        assert kind == ec.VOTERS[name][0], (tag, kind)
        s, b, a = g * P + v, before, o.st
        dt = int(b["current_term"][s]) - int(item["args_term"])
        assert dt == ec.VOTERS[name][2], tag
        if name in ("g_leader_lower",):
            assert b["state"][s] == LEADER and a["state"][s] == FOLLOWER and a["voted_for"][s] == c, tag
        if name in ("e_leader_equal", "h_leader"):
            assert b["state"][s] == LEADER and a["state"][s] == LEADER, tag
        if name == "e_junk_equal":
            assert b["voted_for"][s] == P and a["voted_for"][s] == P, tag
        if name == "g_junk_lower":
            assert b["voted_for"][s] == P and a["voted_for"][s] == c, tag
        if name == "g_again":
            assert b["voted_for"][s] == c and dt == 0, tag
        if name == "e_voted_other":
            assert b["voted_for"][s] not in (-1, c, P) and a["voted_for"][s] == b["voted_for"][s], tag
        if name in ("e_log_term", "e_log_index"):
            assert b["voted_for"][s] == -1 and a["voted_for"][s] == -1, tag
            cl, vl = before["last_index"][g * P + c], before["last_index"][s]
            assert (vl > cl) == (name == "e_log_index") and (vl < cl) == (name == "e_log_term"), tag
        have.add((c, name))
    missing = [f"P {P} c {c}: voter class {n}" for c in range(P) for n in ec.VOTERS if (c, n) not in have]
    assert not missing, missing


def test_directed_table_holds_every_scenario(table):
    case, rec, before, o = table
    P, tags, B = case["P"], case["tags"], case["B"]
    if P not in ec.SCENARIO_P:
        assert all(t[0] in ("tally", "voter") for t in tags)
        return
    by_slot = {int(s): i for i, s in enumerate(rec["slot"])}
    a = o.st
    have = set()
    for g, tag in enumerate(tags):
        name = tag[0]
        if name in ("tally", "voter"):
            continue
        have.add(tag)
        sl = lambda p: g * P + p  # noqa: E731
        if name in ("equal", "high_bits"):
            c1, c2 = tag[1:]
            r1, r2 = by_slot[sl(c1)], by_slot[sl(c2)]
            assert rec["grants"][r1] == P - 2 and rec["grants"][r2] == 0, tag      # the lower peer takes every free vote
            assert rec["guard"][r2] and (rec["items"][r2]["reply_term"] == rec["items"][r2]["args_term"]).all(), tag
            assert a["state"][sl(c1)] == LEADER and a["state"][sl(c2)] == CANDIDATE, tag
            assert a["current_term"][sl(c2)] == B + 1 and a["voted_for"][sl(c2)] == c2, tag
            if name == "high_bits":
                assert int(case["mask"][0][g]) >> P == (0xFF >> P), tag
        elif name == "lower_higher_term":
            c1, c2 = tag[1:]
            r2 = by_slot[sl(c2)]
            assert not rec["guard"][r2], tag                                        # deposed by c1's RequestVote
            assert (rec["items"][r2]["reply_term"] > rec["items"][r2]["args_term"]).all(), tag
            assert not rec["items"][r2]["vote_granted"].any() and not rec["flags"][r2].any(), tag
            assert a["state"][sl(c2)] == FOLLOWER and a["state"][sl(c1)] == LEADER, tag
        elif name == "higher_higher_term":
            c1, c2 = tag[1:]
            r1 = by_slot[sl(c1)]
            assert rec["grants"][r1] >= P // 2 and not rec["guard"][r1] and not rec["flags"][r1].any(), tag
            assert a["granted_votes"][sl(c1)] == 1 and a["state"][sl(c1)] == FOLLOWER, tag
            assert a["state"][sl(c2)] == LEADER, tag
        elif name in ("all_equal", "all_staggered"):
            assert all(sl(p) in by_slot for p in range(P)), tag
        elif name == "leader_bit_deposed":
            c1, c2 = tag[1:]
            assert sl(c1) not in by_slot and sl(c2) in by_slot, tag
            assert before["state"][sl(c1)] == LEADER and a["state"][sl(c1)] == FOLLOWER, tag
            assert a["voted_for"][sl(c1)] == c2, tag
        elif name == "leader_bit_alone":
            c1 = tag[1]
            assert not any(sl(p) in by_slot for p in range(P)), tag
            assert all(np.array_equal(a[k].reshape(case["G"], -1)[g], before[k].reshape(case["G"], -1)[g]) for k in a), tag
        else:
            assert name.startswith("three_") and all(sl(p) in by_slot for p in tag[1:]), tag
            if name != "three_equal":  # the candidate with the highest args.Term deposes the other two
                top = tag[1:][name[6:].index("2")]
                assert [bool(rec["guard"][by_slot[sl(p)]]) for p in tag[1:]] == [p == top for p in tag[1:]], tag
    pairs = [(c1, c2) for c1 in range(P) for c2 in range(c1 + 1, P)]
    want = {(n, c1, c2) for n in ec.SCENARIOS[:3] + ec.SCENARIOS[5:8] for c1, c2 in pairs}
    want |= {("all_equal",), ("all_staggered",)}
    want |= {(n, c1, c2, c3) for n in ec.SCENARIOS[8:] for c1, c2 in pairs for c3 in range(c2 + 1, P)}
    missing = sorted(map(str, want - have))
    assert not missing, missing
    # mask bits at and above P change nothing
    lo = Oracle(case["G"], P, case["L"], case["st"])
    gf = lo.election_rounds(case["mask"] & ((1 << P) - 1))
    hi = Oracle(case["G"], P, case["L"], case["st"])
    assert np.array_equal(gf, hi.election_rounds(case["mask"] | np.uint8((0xFF << P) & 0xFF)))
    assert_states_equal(lo.state(), hi.state(), case["G"], P, case["L"], "mask bits at and above P")


# ---- 3. the edge set ------------------------------------------------------------------------
def test_edge_set_holds_every_log_shape_and_size():
    assert {c[1] for c in ec.EDGE_CASES} == set(ec.EDGE_G)
    assert {c[3] for c in ec.EDGE_CASES} >= {0, 1, 2, 3, 65}
    assert {(c[0], c[2]) for c in ec.EDGE_CASES if c[2] == 1} == {(1, 1), (2, 1)}
    have, slots = set(), set()
    for cs in ec.EDGE_CASES:
        c = ec.edge(*cs)
        P, G, L, R = cs
        assert c["mask"].shape == (R, G)
        if R == 0:
            continue
        st = c["st"]
        cand = np.zeros(G * P, bool)
        cand[ec.candidates_of(st, c["mask"][0], P)] = True
        cg = cand.reshape(G, P).astype(np.int64)
        voter = (cg.sum(axis=1, keepdims=True) - cg > 0).reshape(-1)   # some other replica's RequestVote arrives
        pos = ec.last_entry_slot(st, L)
        live = st["last_index"] > st["dummy_index"]
        for s in range(G * P):
            for who, on in (("candidate", cand[s]), ("voter", voter[s])):
                if on:
                    have.add((L, who, c["kinds"][s]))
                    if live[s]:
                        slots.add((who, "slot 0" if pos[s] == 0 else "slot L-1" if pos[s] == L - 1 else "inside"))
    missing = [f"L {L}: {who} with log {k}" for L in (1, ec.L_SMALL) for who in ("candidate", "voter")
               for k in ec.edge_logs(L) if (L, who, k) not in have]
    missing += [f"{who}: last entry at {w}" for who in ("candidate", "voter") for w in ("slot 0", "slot L-1")
                if (who, w) not in slots]
    assert not missing, missing


def test_high_term_base_stays_in_the_domain():
    """Signed overflow is outside the oracle's domain: no term may reach
    2^31 - 1 within the rounds the GPU tests run (two launches of every mask)."""
    B = ec.BASES[1]
    for case in [ec.exhaustive(2, B)] + [ec.directed(P, B) for P in ec.DIRECTED_P]:
        assert case["st"]["current_term"].min() >= B
        assert ec.max_term_after(case, launches=2) < ec.TERM_MAX, case["name"]


# ---- 5. the references agree with each other ----------------------------------------------------
def _composed_rounds(case):
    """Every round of the case through TimersModel._round, which asserts that
    the message-level composition equals Oracle.election_rounds."""
    G, P, L = case["G"], case["P"], case["L"]
    m = TimersModel(G, P, L, case["st"])
    want = Oracle(G, P, L, case["st"])
    gf = np.zeros(G, np.int32)
    for r in range(case["mask"].shape[0]):
        cand = np.zeros(G * P, bool)
        cand[ec.candidates_of(m.state(), case["mask"][r], P)] = True
        gf |= m._round(cand)[0]
    assert np.array_equal(gf, want.election_rounds(case["mask"]))
    assert_states_equal(m.state(), want.state(), G, P, L, case["name"])


@pytest.mark.parametrize("P,B", [(1, 10), (2, 10), (2, ec.BASES[1]), (3, 10)])
def test_composition_equals_election_rounds_exhaustive(P, B):
    _composed_rounds(ec.exhaustive(P, B))


@pytest.mark.parametrize("B", ec.BASES)
def test_composition_equals_election_rounds_directed_and_edges(B):
    for P in ec.DIRECTED_P:
        _composed_rounds(ec.directed(P, B))
    if B == 10:
        for cs in ec.EDGE_CASES:
            _composed_rounds(ec.edge(*cs))


def _c_vs_py(case):
    G, P, L = case["G"], case["P"], case["L"]
    o = Oracle(G, P, L, case["st"])
    gf = o.election_rounds(case["mask"])
    pst, pgf = py_election_rounds(case["st"], G, P, L, case["mask"])
    assert np.array_equal(gf, pgf), case["name"]
    assert_states_equal(o.state(), pst, G, P, L, case["name"], heads=False)


@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_statement_level_restatement_directed(P):
    _c_vs_py(ec.directed(P))


def test_statement_level_restatement_exhaustive():
    _c_vs_py(ec.exhaustive(2))
    _c_vs_py(ec.exhaustive_subset(3, ec.PY_SUBSET, seed=0x9707))


# ---- 4. the clock step on these states -------------------------------------------------------------
def test_clock_subset_meets_the_leader_situations():
    case = ec.exhaustive_subset(3, ec.CLOCK_SUBSET, seed=0xC10C)
    assert case["G"] <= 65536
    G, P = case["G"], case["P"]
    m = ec.clock_model(case)
    due = (m.ed <= NOW0).reshape(G, P)
    assert np.array_equal(due, ec.mask_bits(case["mask"][0], P)), "the due set at NOW0 is not round 0's mask"
    assert ((m.hd <= NOW0) & (case["st"]["state"] == LEADER)).any(), "no Leader's heartbeat timer is due"
    lead0 = (case["st"]["state"] == LEADER).reshape(G, P)
    out = m.clock_step(NOW0, False)
    assert np.array_equal(out["cand_mask"], ((due & ~lead0) << np.arange(P)).sum(axis=1).astype(np.uint8))
    m.clock_step(NOW0 + 1, False)
    missing = [k for k in ("two_leaders_equal", "two_leaders_diff", "fired_deposed", "grants", "elected")
               if not m.stats[k]]
    assert not missing, (missing, m.stats)


@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_clock_steps_on_the_directed_table_model(P):
    case = ec.directed(P)
    for send_all in (False, True):
        m = ec.clock_model(case)
        for k in range(ec.CLOCK_STEPS):
            m.clock_step(NOW0 + k, send_all)          # _round's self-check runs inside
        assert m.stats["elected"] and m.stats["grants"]
