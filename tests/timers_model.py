"""numpy model of the engine's timers (include/mraft.h "timers"): the
stateless election-timeout draw, ticker(), the seven reset sites and the clock
step, built on the CPU oracle (oracle_lib.Oracle) and on nothing of the
engine's timer code. Test infrastructure only.

The clock step's election round is composed from the oracle's message-level
calls (compose_round: start_election for the candidates in peer order,
handle_request_vote candidate rank by candidate rank — distinct voter slots
per call — then process_vote_replies in voter order; the composition takes any
object with those three methods, so the GPU tests run it on an Engine too),
which yields the per-voter grants the timers need; the model asserts that this composition equals
Oracle.election_rounds on a copy of the state. The tick is Oracle.replicate_tick.
"""
from __future__ import annotations

import numpy as np

from multiraft_amd import _abi
from multiraft_amd._abi import LEADER, RV_ARGS, RV_RESULT
from multiraft_amd.engine import new_state
from oracle_lib import Oracle

NOW_MAX = 1 << 30
ELECTION_MAX = 1 << 20


def fmix(h):
    h = np.asarray(h, dtype=np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def config_ok(heartbeat, lo, hi):
    return 1 <= heartbeat < (1 << 30) and 1 <= lo < hi <= ELECTION_MAX


def draw(seed, slot, now, lo, hi):
    """election_lo + fmix(fmix(slot * 0x9E3779B9 + now) ^ seed) % (hi - lo), in
    uint32 arithmetic (carried in uint64 and masked)."""
    slot = np.asarray(slot, dtype=np.uint64)
    h = fmix((slot * 0x9E3779B9 + np.uint64(now)) & 0xFFFFFFFF)
    h = fmix(h ^ np.uint64(seed & 0xFFFFFFFF))
    return (lo + (h % np.uint64(hi - lo))).astype(np.int64)


def deliver_round(node, G, P, cslots):
    """The first two legs of one election round on `node` (any object with
    start_election and handle_request_vote: the Oracle, an Engine):
    start_election for the candidates `cslots` (ascending slots), then one
    handle_request_vote call per candidate rank within its group (distinct
    voter slots per call). Returns (items, seg, granted): the RV_RESULT records
    in voter order within each candidate with their segment bounds for
    process_vote_replies (None when P < 2 or nobody timed out), and
    granted[G*P], the voters that granted another replica's RequestVote."""
    granted = np.zeros(G * P, bool)
    if not len(cslots):
        return None, None, granted
    args, err = node.start_election(cslots)
    assert not err.any()
    if P < 2:
        return None, None, granted
    grp = cslots // P
    rank = np.arange(len(cslots)) - np.searchsorted(grp, grp)  # rank within its group
    res = np.zeros((len(cslots), P), dtype=RV_RESULT)
    for k in range(int(rank.max()) + 1):
        idx = np.nonzero(rank == k)[0]
        c = cslots[idx]
        voters = np.arange(P)[None, :].repeat(len(idx), 0)
        keep = voters != (c % P)[:, None]
        vs = ((c // P)[:, None] * P + voters)[keep]
        a = np.zeros(len(vs), dtype=RV_ARGS)
        src = np.repeat(idx, P - 1)
        a["slot"] = vs
        a["candidate_id"] = cslots[src] % P
        for f in ("term", "last_log_index", "last_log_term"):
            a[f] = args[f][src]
        rep, herr = node.handle_request_vote(a)
        assert not herr.any()
        granted[vs[rep["vote_granted"] != 0]] = True
        r = res[src, vs % P]
        r["slot"], r["peer"] = cslots[src], vs % P
        r["args_term"], r["reply_term"], r["vote_granted"] = a["term"], rep["term"], rep["vote_granted"]
        res[src, vs % P] = r
    keep = np.arange(P)[None, :] != (cslots % P)[:, None]
    items = res[keep]                                  # voter order within each candidate
    seg = np.arange(len(cslots) + 1, dtype=np.int64) * (P - 1)
    return items, seg, granted


def tally_round(node, G, P, items, seg):
    """The third leg: one process_vote_replies call over deliver_round's
    records. Returns (group flags, became[G*P], the per-item flags)."""
    became = np.zeros(G * P, bool)
    gf = np.zeros(G, np.int32)
    if items is None:
        return gf, became, np.zeros(0, np.int32)
    fl, terr = node.process_vote_replies(items, seg)
    assert not terr.any()
    lead = (fl & _abi.F_BECAME_LEADER) != 0
    became[items["slot"][lead]] = True
    np.bitwise_or.at(gf, items["slot"][lead] // P, _abi.G_ELECTED)
    sd = (fl & _abi.F_STEPPED_DOWN) != 0
    np.bitwise_or.at(gf, items["slot"][sd] // P, _abi.G_STEPPED_DOWN)
    return gf, became, fl


def compose_round(node, G, P, cslots):
    """One election round from the message-level calls on `node`:
    (group flags, granted[G*P], became[G*P])."""
    items, seg, granted = deliver_round(node, G, P, cslots)
    gf, became, _ = tally_round(node, G, P, items, seg)
    return gf, granted, became


class TimersModel:
    def __init__(self, G, P, L, st=None):
        self.G, self.P, self.L = G, P, L
        self.o = Oracle(G, P, L, new_state(G, P, L) if st is None else st)
        self.ed = self.hd = None
        self.cfg = None
        # how often the clock step met the situations the GPU tests must cover
        self.stats = dict(two_leaders_diff=0, two_leaders_equal=0, fired_deposed=0, sender_stepped_down=0,
                          need_snapshot=0, grants=0, elected=0)

    # ---- state ---------------------------------------------------------------
    def state(self):
        return self.o.state()

    def timers(self):
        return self.ed.copy(), self.hd.copy()

    def _slots(self):
        return np.arange(self.G * self.P, dtype=np.int64)

    def _edl(self, slots, now):
        seed, _, lo, hi = self.cfg
        return (now + draw(seed, slots, now, lo, hi)).astype(np.int32)

    def enable(self, seed, heartbeat, lo, hi, now=0):
        assert config_ok(heartbeat, lo, hi) and 0 <= now <= NOW_MAX
        self.cfg = (seed, heartbeat, lo, hi)
        self.ed = self._edl(self._slots(), now)
        self.hd = np.full(self.G * self.P, now + heartbeat, np.int32)

    def load(self, ed=None, hd=None):
        if ed is not None:
            self.ed = np.array(ed, dtype=np.int32)
        if hd is not None:
            self.hd = np.array(hd, dtype=np.int32)

    def arm(self, slots, now):
        s = np.asarray(slots, dtype=np.int64)
        s = s[(s >= 0) & (s < self.G * self.P)]
        self.ed[s] = self._edl(s, now)
        self.hd[s] = now + self.cfg[1]

    # ---- ticker (raft.go:106-125) ----------------------------------------------
    def ticker(self, now, cap_e=None, cap_h=None):
        gp = self.G * self.P
        cap_e = gp if cap_e is None else cap_e
        cap_h = gp if cap_h is None else cap_h
        leader = self.o.st["state"] == LEADER
        edue, hdue = self.ed <= now, self.hd <= now
        le = np.nonzero(edue & ~leader)[0]
        lh = np.nonzero(hdue & leader)[0]
        keep_e = np.zeros(gp, bool)
        keep_e[le[cap_e:]] = True     # listed, not written: stays due
        keep_h = np.zeros(gp, bool)
        keep_h[lh[cap_h:]] = True
        re_ = np.nonzero(edue & ~keep_e)[0]
        self.ed[re_] = self._edl(re_, now)
        self.hd[hdue & ~keep_h] = now + self.cfg[1]
        return le[:cap_e].astype(np.int32), len(le), lh[:cap_h].astype(np.int32), len(lh)

    # ---- the reset sites of the message path ------------------------------------
    def note(self, kind, records, outcome, item_err, now):
        n = len(records)
        ok = np.ones(n, bool) if item_err is None else (np.asarray(item_err) == 0)
        slot = records["slot"].astype(np.int64)
        if kind in (_abi.NOTE_AE_HANDLED, _abi.NOTE_IS_HANDLED):
            hit = outcome["term"] <= records["term"]
        elif kind == _abi.NOTE_RV_HANDLED:
            hit = outcome["vote_granted"] != 0
        elif kind in (_abi.NOTE_AE_FOLDED, _abi.NOTE_IS_FOLDED):
            hit = (np.asarray(outcome) & _abi.F_STEPPED_DOWN) != 0
        else:
            hit = (np.asarray(outcome) & _abi.F_BECAME_LEADER) != 0
        s = slot[ok & hit & (slot >= 0) & (slot < self.G * self.P)]
        if kind == _abi.NOTE_RV_FOLDED:
            self.hd[s] = now + self.cfg[1]
        else:
            self.ed[s] = self._edl(s, now)

    # ---- one election round from the message-level calls ---------------------------
    def _round(self, cand):
        """cand: bool[G*P], the replicas that time out (non-leaders). Returns
        (group flags, granted[G*P]: the voter granted another replica's
        RequestVote, became[G*P])."""
        G, P, o = self.G, self.P, self.o
        check = Oracle(G, P, self.L, o.st)
        check.st["terms_sorted"][:] = o.st["terms_sorted"]
        gf, granted, became = compose_round(o, G, P, np.nonzero(cand)[0].astype(np.int32))
        # the composition is the storm's round
        bits = (cand.reshape(G, P).astype(np.int64) << np.arange(P)).sum(axis=1).astype(np.uint8)
        cgf = check.election_rounds(bits[None, :])
        assert np.array_equal(gf, cgf), "composed round: flags differ from election_rounds"
        for k, v in o.st.items():
            assert np.array_equal(v, check.st[k]), f"composed round: {k} differs from election_rounds"
        return gf, granted, became, bits

    # ---- the clock step ----------------------------------------------------------------
    def clock_step(self, now, send_all=False):
        G, P, o = self.G, self.P, self.o
        hb = self.cfg[1]
        slots = self._slots()
        dl = self._edl(slots, now)
        role0 = o.st["state"].copy()
        # A
        edue, hdue = self.ed <= now, self.hd <= now
        self.ed[edue] = dl[edue]
        cand = edue & (role0 != LEADER)
        fired = hdue & (role0 == LEADER)
        self.hd[hdue & (role0 != LEADER)] = now + hb
        # B
        eflags, granted, became, bits = self._round(cand)
        self.ed[granted] = dl[granted]
        self.hd[became] = now + hb
        # C
        role1 = o.st["state"]
        elig = (role1 == LEADER) & (fired | became | bool(send_all))
        term = o.st["current_term"].astype(np.int64)
        key = np.where(elig, term * 8 + (7 - slots % P), -1).reshape(G, P)  # highest term, then lowest peer
        best = key.argmax(axis=1)
        has = key.max(axis=1) >= 0
        lp = np.where(has, best, -1).astype(np.int32)
        sender = (np.arange(G) * P + np.maximum(lp, 0))
        tg = np.where(has, term[sender], 0)
        self.hd[sender[has]] = now + hb
        # what happened (for the tests that must cover these situations)
        ne = elig.reshape(G, P).sum(axis=1)
        for g in np.nonzero(ne >= 2)[0]:
            t = term.reshape(G, P)[g][elig.reshape(G, P)[g]]
            self.stats["two_leaders_equal" if (t == t.max()).sum() >= 2 else "two_leaders_diff"] += 1
        self.stats["fired_deposed"] += int((fired & (role1 != LEADER)).sum())
        self.stats["grants"] += int(granted.sum())
        self.stats["elected"] += int(became.sum())
        # D
        gf = o.replicate_tick(lp)
        commit, tl = o.export_group_status(lp)
        # E
        live = ((gf & _abi.G_ACTIVE) != 0) & ((gf & _abi.G_ERROR) == 0)
        term2 = o.st["current_term"].reshape(G, P)
        is_sender = np.arange(P)[None, :] == lp[:, None]
        hit = live[:, None] & np.where(is_sender, ((gf & _abi.G_STEPPED_DOWN) != 0)[:, None],
                                       term2 == tg[:, None])
        hit = hit.reshape(-1)
        self.ed[hit] = dl[hit]
        self.stats["sender_stepped_down"] += int((live & ((gf & _abi.G_STEPPED_DOWN) != 0)).sum())
        self.stats["need_snapshot"] += int((live & ((gf & _abi.G_NEED_SNAPSHOT) != 0)).sum())
        return dict(cand_mask=bits, leader_peer=lp, election_flags=eflags, group_flags=gf, commit=commit,
                    term_leader=tl)


# ---- the self-driving scenario (test_test.go TestInitialElection / TestReElection) ----------
SELF_CFG = dict(seed=1, heartbeat=9, lo=30, hi=60)
SELF_SHAPES = ((64, 3), (64, 5), (64, 2), (33, 1))
SELF_L = 64


def leaders_per_group(st, G, P):
    return (st["state"].reshape(G, P) == LEADER).sum(axis=1)


def restart(node, slots, now):
    """Crash + restart of the replicas `slots` from their persisted state, then
    Make's two timers (`node`: an Engine, or a ModelNode)."""
    hdr, terms = node.read_persistent(slots)
    err = node.restore(hdr, terms)
    assert not err.any()
    node.timers_arm(slots, now)


class ModelNode:
    """The model behind the Engine's method names, for scenarios driven through
    either."""

    def __init__(self, model: TimersModel):
        self.m = model
        self.G, self.P, self.L = model.G, model.P, model.L
        # the message-level calls of the host-driven sequence (tests/timers_sequence.py)
        o = model.o
        self.start_election, self.handle_request_vote, self.process_vote_replies = (
            o.start_election, o.handle_request_vote, o.process_vote_replies)
        self.gather_append_args, self.handle_append_entries, self.process_append_replies = (
            o.gather_append_args, o.handle_append_entries, o.process_append_replies)
        self.election_rounds = o.election_rounds

    def ticker(self, now, cap_e=None, cap_h=None):
        return self.m.ticker(now, cap_e, cap_h)

    def timers_enable(self, seed, heartbeat, election_lo, election_hi, now=0):
        self.m.enable(seed, heartbeat, election_lo, election_hi, now)

    def timers_note(self, kind, records, outcome, item_err, now):
        self.m.note(kind, records, outcome, item_err, now)

    def load_state(self, st):
        self.m.o.load_state(st)

    def store_state(self):
        return self.m.o.store_state()

    def timers_load(self, election_due=None, heartbeat_due=None):
        self.m.load(election_due, heartbeat_due)

    def timers_store(self):
        return self.m.timers()

    def read_persistent(self, slots):
        return self.m.o.read_persistent(slots)

    def restore(self, hdr, terms):
        return self.m.o.restore(hdr, terms)

    def timers_arm(self, slots, now):
        self.m.arm(slots, now)

    def start(self, slots, counts):
        return self.m.o.start(slots, counts)

    def clock_step(self, now, send_all=False):
        return self.m.clock_step(now, send_all)

    def scalar_state(self):
        return self.m.o.st


def start_plan(G, P, tick, st):
    """Leg three: 1-4 entries at every group's Leader on every third tick
    (deterministic in the tick)."""
    if tick % 3:
        return None
    slots = np.nonzero(st["state"] == LEADER)[0].astype(np.int32)
    counts = (1 + (slots + tick) % 4).astype(np.int32)
    return slots, counts


def self_driving(nodes, G, P, check=None, t_end1=300, leg3=40):
    """The self-driving run on every node of `nodes` in lockstep (the first is
    the model's ModelNode, whose state plans the restarts and the Starts):
    leg 1 from Make state, clock_step for now = 1..t_end1; leg 2, every
    group's Leader crashes and restarts at t_end1, then 2 * election_hi more
    ticks; leg 3, `leg3` ticks with Start at the Leaders between steps and
    MRAFT_CLOCK_SEND_ALL. check(tick, outs) runs after every step with every
    node's outputs. Returns the model's history: per tick (leaders per group,
    terms, commit output)."""
    hist = {}
    ref = nodes[0]

    def step(t, send_all=False):
        outs = [n.clock_step(t, send_all) for n in nodes]
        if check:
            check(t, outs)
        st = ref.scalar_state()
        hist[t] = (leaders_per_group(st, G, P), st["current_term"].copy(), outs[0]["commit"].copy(),
                   outs[0]["election_flags"].copy())

    for t in range(1, t_end1 + 1):
        step(t)
    slots = np.nonzero(ref.scalar_state()["state"] == LEADER)[0].astype(np.int32)  # every group's Leader
    if len(slots):
        for n in nodes:
            restart(n, slots, t_end1)
    t2 = t_end1 + 2 * SELF_CFG["hi"]
    for t in range(t_end1 + 1, t2 + 1):
        step(t)
    for t in range(t2 + 1, t2 + leg3 + 1):
        plan = start_plan(G, P, t, ref.scalar_state())
        if plan is not None and len(plan[0]):
            got = [n.start(*plan) for n in nodes]
            for g in got[1:]:
                for a, b in zip(g, got[0]):
                    assert np.array_equal(a, b), (t, "start")
        step(t, send_all=True)
    return hist
