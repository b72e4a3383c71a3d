"""Directed cases and schedules of the in-place crash (mraft_crash;
tests/test_crash_cases.py on the CPU, tests/test_crash_gpu.py on the engine).
Test infrastructure only.

  R  reset      hand-placed replicas (snapshot_matrix_cases.Reps) in every
                role, with every volatile field away from its Make value, and
                batches of 0 .. 257 items with a slot twice, slots -1 and G*P
                and item_err NULL. Loaded with mraft_load_state.
  T  the proof  long rows around the 64-lane and 256-term edges of the ring
                scan, with terms_sorted withheld (bound as is, mraft_bind_state)
                over sorted terms, one descent per row, and the proof kept.
  B  bounds     last < dummy and last - dummy = L, bound as is.

A family is a dict: G, P, L, st (the state image), srt (the terms_sorted
array the engine is bound with; None: the family is loaded and the engine
computes it), batches [(slots, null_err)] and for T and B the expectation per
replica. Every batch runs on the family's initial state.

The schedules (SCENARIOS) are reach_cases' extended with crash and restart: a
phase is a function (P, L, M, up) -> (up', conn): who is up after the phase's
crashes and restarts and who is connected among them.

Run as a program: every family on the library MRAFT_LIB names against the
model, one JSON line {"cases": [[name, n_items, ok], ...]}, exit status 1 on
any mismatch."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from cases_program import run_all  # noqa: E402
from crash_model import CrashModel, assert_log_untouched  # noqa: E402
from oracle_lib import assert_states_equal, logical_logs  # noqa: E402
from reach_cases import SCEN_CFG, SCEN_L, SCEN_PHASE  # noqa: E402,F401
from snapshot_matrix_cases import DESCENTS, ROW_LENS, WRAPS, Reps  # noqa: E402

from multiraft_amd._abi import (CANDIDATE, FOLLOWER, ITEM_BAD_SLOT, ITEM_BAD_STATE, LEADER,  # noqa: E402
                                STATE_FIELDS)

R_SHAPES = [(P, L) for P in (1, 2, 3, 5, 8) for L in (16, 13)]
R_G = 64
BATCH_SIZES = (0, 1, 4, 5, 63, 64, 65, 257)     # 257: four waves per workgroup and one item more than 64 of them
NULL_ERR_SIZES = (5, 65)
T_LS = (520, 515)
T_DESCENTS = DESCENTS + ((0, 1),)                # (0, 1): the dummy is outside the rule
ROLES = (LEADER, CANDIDATE, FOLLOWER)


# ---------------------------------------------------------------- R
def r_replica(s, P, L):
    """The placement of replica slot s of an R family (Reps.put's arguments)."""
    me = s % P
    role = ROLES[s % 3]
    n = (0, 1, L - 1, 3, L // 2)[s % 5]                     # an empty log ... a full ring
    head = (0, L // 2, L - 1)[(s // 3) % 3]
    dummy = (0, 9)[(s // 5) % 2]
    voted = (-1, me, (me + 1) % P, P)[(s // 2) % 4]         # (P: junk; at P = 1 "other" is the replica itself)
    log = [2 + (3 * i) // max(n, 1) for i in range(n)]      # terms 2 .. 4, never decreasing
    if s % 11 == 0 and n >= 3:
        log[1] = 9                                          # one descent: no proof for this one
    commit = dummy + min(n, s % 4)
    applied = dummy + (commit - dummy) // 2
    match = {j: dummy + (j + s) % (n + 1) for j in range(P)} if (role == LEADER or s % 2) else None
    nxt = {j: dummy + 1 + (j + 2 * s) % (n + 1) for j in range(P)} if (role == LEADER or s % 4 == 1) else None
    return dict(log=log, T=12, role=role, dummy=dummy, dterm=1 if dummy else 0, head=head, commit=commit,
                applied=applied, voted=voted, match=match, nxt=nxt, hsnap=(s // 7) % 2, dirty=(s // 3) % 4,
                votes=(s % 3) if role != FOLLOWER else (s // 9) % 2)


def batch_slots(n, gp, k):
    """n slots dealt with a stride coprime to gp from an offset that follows k;
    from 4 items on, item 1 is -1, item 2 is G*P and item 3 repeats item 0.
    More items than replicas repeat slots too."""
    stride = next(c for c in (7, 11, 13, 17, 19, 23) if np.gcd(c, gp) == 1)
    s = ((5 * k + np.arange(n, dtype=np.int64) * stride) % gp).astype(np.int32)
    if n >= 4:
        s[1], s[2], s[3] = -1, gp, s[0]
    return s


def fam_r(P, L):
    G = R_G
    reps = Reps(P, L)
    for g in range(G - 1):                                  # the last group stays as Make left it
        reps.group()
        for p in range(P):
            reps.put(g, p, **r_replica(g * P + p, P, L))
    st = reps.state(G)
    batches = [(batch_slots(n, G * P, k), n in NULL_ERR_SIZES) for k, n in enumerate(BATCH_SIZES)]
    return dict(G=G, P=P, L=L, st=st, srt=None, batches=batches)


# ---------------------------------------------------------------- T
def t_rows(L):
    """(entries, wrap, kind, descent) of every T row: kind "withheld" (sorted
    terms, proof 0 -> 1), "kept" (proof 1 -> 1), "descent" (proof 0 -> 0, or
    -> 1 for the pair (0, 1))."""
    rows = []
    for n in ROW_LENS + (L - 1,):
        for w in WRAPS:
            if w > n:
                continue
            rows.append((n, w, "withheld", None))
            rows.append((n, w, "kept", None))
            rows += [(n, w, "descent", d) for d in T_DESCENTS if d[1] <= n]
    return rows


def fam_t(L):
    P = 2
    rows = t_rows(L)
    reps = Reps(P, L)
    srt, expect = [], []
    for k, (n, w, kind, d) in enumerate(rows):
        if k % P == 0:
            reps.group()
        log = [2 + i // 64 for i in range(1, n + 1)]        # entry i (Index dummy + i): sorted
        dterm = 1
        want = 1
        if kind == "descent":
            if d == (0, 1):
                dterm = 100                                 # dummy above entry 1: still sorted after the dummy
            else:
                log[d[0] - 1] += 20                         # entry d[0] above entry d[1]: the row's one descent
                want = 0
        # entry w sits at ring position 0 (w = 0: head 0, no wrap)
        reps.put(k // P, k % P, log=log, T=60, role=ROLES[k % 3], dummy=(0, 1000)[k % 2], dterm=dterm,
                 head=(L - w) % L, commit=(0, 1000)[k % 2] + min(n, 1), applied=(0, 1000)[k % 2], votes=k % 2)
        srt.append(1 if kind == "kept" else 0)
        expect.append(want)
    G = len(reps.groups)
    st = reps.state(G)
    gp = G * P
    srt = np.array(srt + [0] * (gp - len(rows)), np.int32)
    expect = np.array(expect + [1] * (gp - len(rows)), np.int32)
    assert not (srt & (st["terms_sorted"] == 0)).any(), "a kept proof must be sound"
    keep = np.arange(gp) % 9 == 4                           # not named: bit-identical, the proof still withheld
    slots = np.nonzero(~keep)[0].astype(np.int32)
    return dict(G=G, P=P, L=L, st=st, srt=srt, batches=[(slots, False)], rows=rows, expect=expect)


# ---------------------------------------------------------------- B
def fam_b():
    """Through mraft_bind_state, which takes the arrays as they are: replica 1
    with last < dummy, replica 4 with last - dummy = L; the others sound."""
    G, P, L = 4, 3, 16
    reps = Reps(P, L)
    for g in range(G):
        reps.group()
        for p in range(P):
            reps.put(g, p, **r_replica(g * P + p + 1, P, L))
    st = reps.state(G)
    st["dummy_index"][1], st["last_index"][1] = 5, 4
    st["dummy_index"][4], st["last_index"][4] = 2, 2 + L
    for s in (1, 4):
        st["commit_index"][s] = st["last_applied"][s] = st["dummy_index"][s] + 1
        st["state"][s], st["granted_votes"][s], st["has_snapshot"][s], st["persist_dirty"][s] = LEADER, 2, 1, 3
        st["match_index"][s * P:(s + 1) * P] = 7
        st["next_index"][s * P:(s + 1) * P] = 8
    srt = st["terms_sorted"].copy()
    srt[[1, 4]] = 0
    expect_err = np.zeros(G * P, np.int32)
    expect_err[[1, 4]] = ITEM_BAD_STATE
    return dict(G=G, P=P, L=L, st=st, srt=srt, batches=[(np.arange(G * P, dtype=np.int32), False)], broken=[1, 4],
                expect_err=expect_err)


FAMILIES = ([(f"R{P}_{L}", fam_r, (P, L)) for P, L in R_SHAPES] + [(f"T{L}", fam_t, (L,)) for L in T_LS] +
            [("B", fam_b, ())])
NAMES = [f[0] for f in FAMILIES]
_cache = {}


def family(name):
    """Built once; callers must not modify it."""
    if name not in _cache:
        _, fn, args = next(f for f in FAMILIES if f[0] == name)
        _cache[name] = fn(*args)
    return _cache[name]


def n_items(name):
    return int(sum(len(s) for s, _ in family(name)["batches"]))


def model_for(fam):
    """The family's model in the engine's initial state: the oracle computes
    terms_sorted exactly, a bound engine holds what it was given."""
    m = CrashModel(fam["G"], fam["P"], fam["L"], fam["st"])
    if fam["srt"] is not None:
        m.o.st["terms_sorted"][:] = fam["srt"]
    return m


def good_slots(slots, err):
    return np.unique(np.asarray(slots)[np.asarray(err) == 0])


def check_batch(fam, slots, err, before, after, m, ctx):
    """One crash call's result: `err` (None: item_err was NULL) and the state
    `after` against the model `m` that ran the same call, the log untouched,
    every replica not named (or rejected) bit-identical to `before`."""
    G, P, L = fam["G"], fam["P"], fam["L"]
    want = m.last_err
    if err is not None:
        assert np.array_equal(err, want), (ctx, "item_err", np.nonzero(err != want)[0][:8])
    assert_states_equal(after, m.state(), G, P, L, ctx, heads=False)
    assert_log_untouched(before, after, ctx)
    same = np.ones(G * P, bool)
    same[good_slots(slots, want)] = False
    for k in STATE_FIELDS:
        if k == "log_term":
            continue
        a, b = after[k], before[k]
        if k in ("match_index", "next_index"):
            a, b = a.reshape(G * P, P)[same], b.reshape(G * P, P)[same]
        else:
            a, b = a[same], b[same]
        assert np.array_equal(a, b), (ctx, k, "a replica not named was written")
    if "expect" in fam:                                      # T: the proof's expected value per crashed replica
        g = good_slots(slots, want)
        assert np.array_equal(after["terms_sorted"][g], fam["expect"][g]), (ctx, "terms_sorted")
        assert np.array_equal(after["terms_sorted"][same], fam["srt"][same]), (ctx, "a withheld proof not named")
    if "expect_err" in fam:
        assert np.array_equal(want, fam["expect_err"][slots]), (ctx, "expected BAD_STATE")


def crash_on_model(m, slots):
    m.last_err = m.crash(slots)
    return m.last_err


def run_family_model(name):
    """Every batch of the family on the model alone, checked against the call's
    definition stated directly (not through restore): the reset fields, the
    fields that stay, the errors."""
    fam = family(name)
    G, P, L = fam["G"], fam["P"], fam["L"]
    for bi, (slots, _) in enumerate(fam["batches"]):
        m = model_for(fam)
        before = m.o.store_state()
        err = crash_on_model(m, slots)
        after = m.o.store_state()
        gp = G * P
        bad = (slots < 0) | (slots >= gp)
        assert (err[bad] == ITEM_BAD_SLOT).all() and not (err[~bad] == ITEM_BAD_SLOT).any()
        g = good_slots(slots, err)
        assert (after["state"][g] == FOLLOWER).all()
        for k in ("commit_index", "last_applied"):
            assert np.array_equal(after[k][g], before["dummy_index"][g])
        for k in ("granted_votes", "has_snapshot", "persist_dirty"):
            assert not after[k][g].any()
        for k in ("match_index", "next_index"):
            assert not after[k].reshape(gp, P)[g].any()
        for k in ("current_term", "voted_for", "dummy_index", "last_index"):
            assert np.array_equal(after[k], before[k])
        after["log_head"][:] = before["log_head"]            # the model's restore starts a new ring
        check_batch(fam, slots, None, before, {**after, "log_term": before["log_term"]}, m, f"{name} batch {bi} (model)")
    return n_items(name)


class Bound:
    """An engine on the family's state: loaded (srt None) or bound to device
    tensors as they are. reset() puts the initial state back; state() reads all
    of it to the host."""

    def __init__(self, fam, engine_cls):
        self.fam = fam
        G, P, L = fam["G"], fam["P"], fam["L"]
        self.d = None
        if fam["srt"] is None:
            self.e = engine_cls(G, P, L)
        else:
            import torch
            self.e = engine_cls(G, P, L, alloc=False)
            self.d = {k: torch.from_numpy(np.ascontiguousarray(v, np.int32).copy()).to("cuda:0")
                      for k, v in self._image().items()}
            self.e.bind(self.d)
        self.reset()

    def _image(self):
        return dict(self.fam["st"], terms_sorted=self.fam["srt"]) if self.fam["srt"] is not None else self.fam["st"]

    def reset(self):
        if self.d is None:
            self.e.load_state(self.fam["st"])
        else:
            import torch
            self.e.synchronize()
            for k, v in self._image().items():
                self.d[k].copy_(torch.from_numpy(np.ascontiguousarray(v, np.int32)))
            torch.cuda.synchronize()

    def state(self):
        if self.d is None:
            return self.e.store_state()
        self.e.synchronize()
        return {k: v.cpu().numpy() for k, v in self.d.items()}

    def close(self):
        self.e.close()


def run_family(name, engine_cls):
    """Every batch of the family on an engine against the model."""
    fam = family(name)
    b = Bound(fam, engine_cls)
    try:
        for bi, (slots, null_err) in enumerate(fam["batches"]):
            ctx = f"{name} batch {bi} ({len(slots)} items)"
            b.reset()
            m = model_for(fam)
            before = b.state()
            assert_states_equal(before, m.state(), fam["G"], fam["P"], fam["L"], ctx + ": before the call")
            err = b.e.crash(slots, out=(None,)) if null_err else b.e.crash(slots)
            assert null_err == (err is None)
            crash_on_model(m, slots)
            check_batch(fam, slots, err, before, b.state(), m, ctx)
    finally:
        b.close()
    return n_items(name)


# ---------------------------------------------------------------- schedules
# The reference's crash tests (src/raft/test_test.go:685-871) as phases of
# 2 * election_hi ticks under reach_cases.SCEN_CFG. A phase is a function
# (P, L, M, up) -> (up', conn): L the group's visible Leader when the phase
# begins (-1: none), M the leader remembered from the phase marked "mark", up
# the bit mask of the replicas that are running. The replicas of up & ~up' are
# crashed, those of up' & ~up restarted, and the mask set is conn & up'.
def _bits(P, *peers):
    return sum(1 << (p % P) for p in set(p % P for p in peers))


def _all_up(P, L, M, up):
    return (1 << P) - 1, (1 << P) - 1


def _restart_all(P, L, M, up):
    """crash1 of every replica, then start1 of every replica, in one tick."""
    return "bounce", (1 << P) - 1


def _crash_leader(*offs):
    def fn(P, L, M, up):
        full = (1 << P) - 1
        return (up & ~_bits(P, *(L + o for o in offs)) if L >= 0 else up), full
    return fn


def _up_marked(down=(), cut=()):
    """Everyone up but M + down; M + cut disconnected."""
    def fn(P, L, M, up):
        full = (1 << P) - 1
        return full & ~(_bits(P, *(M + o for o in down)) if down else 0), full & ~(_bits(P, *(M + o for o in cut)) if cut else 0)
    return fn


def _cut_leader(*offs):
    def fn(P, L, M, up):
        full = (1 << P) - 1
        return up, full & ~_bits(P, *(max(L, 0) + o for o in offs))
    return fn


def _figure8(P, L, M, up):
    """Crash the Leader; when fewer than a majority are up, restart the lowest
    replica that is down (other than the one that just crashed)."""
    full = (1 << P) - 1
    if L >= 0:
        up &= ~(1 << L)
    while bin(up).count("1") <= P // 2:
        up |= next(1 << p for p in range(P) if not up >> p & 1 and p != L)
    return up, full


SCENARIOS = {
    # TestPersist12C: crash and restart everyone; the leader; the leader and one follower (no quorum)
    "Persist1": (3, [(_all_up, False), (_restart_all, False), (_crash_leader(0), False), (_all_up, False),
                     (_crash_leader(0, 1), False), (_all_up, False)]),
    # TestPersist22C: rolling crashes of five: two followers down; then the other three while the
    # two come back (no quorum); one more back (quorum); everyone
    "Persist2": (5, [(_all_up, False), (_crash_leader(1, 2), True), (_up_marked(down=(0, 3, 4)), False),
                     (_up_marked(down=(0, 4)), False), (_all_up, False)]),
    # TestPersist32C: the leader's partner cut off; leader and the other follower crash while it
    # reconnects (alone); the leader restarts; everyone
    "Persist3": (3, [(_all_up, False), (_cut_leader(2), True), (_up_marked(down=(0, 1)), False),
                     (_up_marked(down=(1,)), False), (_all_up, False)]),
    # TestFigure82C: the Leader crashes in every phase
    "Figure8": (5, [(_all_up, False)] + [(_figure8, False)] * 5 + [(_all_up, False)]),
}
SCEN_START_EVERY = 4


def scenario_groups(P, G):
    names = [n for n, (p, _) in SCENARIOS.items() if p == P]
    return [names[g % len(names)] for g in range(G)]


def run_scenarios(P, G, engine=None):
    """The schedules of P replicas, one per group and shifted by its index, on
    the model (and with `engine`, an Engine, in lockstep, every output and the
    whole state compared after every call), driven by set_reachable, crash,
    timers_arm, start, clock_step and the compacted applier only. Asserts the
    reference's conditions and returns what happened, counted."""
    from reach_cases import visible_leader
    from reach_model import connected

    L = SCEN_L
    cfg, W = SCEN_CFG, SCEN_PHASE
    names = scenario_groups(P, G)
    shift = np.arange(G) % cfg["lo"]
    m = CrashModel(G, P, L)
    m.enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], 0)
    e = engine
    if e is not None:
        e.timers_enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], 0)
    full = (1 << P) - 1
    up = np.full(G, full, np.int64)
    conn_want = np.full(G, full, np.int64)
    marked = np.zeros(G, np.int64)
    phase = np.full(G, -1)
    leader_of_term = [dict() for _ in range(G)]
    applied = [dict() for _ in range(G)]
    applied_by = [dict() for _ in range(G * P)]       # slot -> Index -> term: what each replica applied, ever
    phase_commit = np.zeros(G, np.int64)
    n_phase = max(len(s[1]) for n, s in SCENARIOS.items() if s[0] == P)
    c = dict(majority_leader=0, no_quorum=0, agree=0, reapplied=0, crashes=0, restarts=0, bounce=0, down_ticks=0,
             leader_crashed=0, elected_after_crash=0)
    outs = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")

    def both(ctx):
        if e is None:
            return
        assert_states_equal(e.store_state(), m.state(), G, P, L, ctx, heads=False)
        for name, a, b in zip(("election_due", "heartbeat_due"), e.timers_store(), (m.ed, m.hd)):
            assert np.array_equal(a, b), (ctx, name, np.nonzero(a != b)[0][:8])

    def crash(slots, ctx):
        slots = np.asarray(slots, np.int32)
        want = m.crash(slots)
        assert not want.any()
        if e is not None:
            before = e.store_state()
            assert np.array_equal(e.crash(slots), want), ctx
            assert_log_untouched(before, e.store_state(), ctx)

    def arm(slots, now):
        slots = np.asarray(slots, np.int32)
        m.arm(slots, now)
        if e is not None:
            e.timers_arm(slots, now)

    for t in range(1, n_phase * W + int(shift.max()) + 1):
        stt = m.state()
        role, term = stt["state"].reshape(G, P), stt["current_term"].reshape(G, P)
        commit = stt["commit_index"].reshape(G, P)
        to_crash, to_arm = [], []
        for g in range(G):
            sched = SCENARIOS[names[g]][1]
            k = (t - 1 - shift[g]) // W
            if k == phase[g] or k < 0:
                continue
            reach_g = int(up[g] & conn_want[g])
            live = [p for p in range(P) if reach_g >> p & 1]
            if phase[g] >= 0:                                # the phase that ends: its conditions
                lead = [p for p in live if role[g, p] == LEADER]
                if len(live) > P // 2:
                    assert lead, (names[g], g, "no Leader among an up-and-connected majority", int(phase[g]), t)
                    c["majority_leader"] += 1
                else:
                    assert max((commit[g, p] for p in range(P) if up[g] >> p & 1), default=0) <= phase_commit[g], \
                        (names[g], g, "commit advanced without a majority")
                    c["no_quorum"] += 1
            phase[g] = k
            Lg = visible_leader(role[g], term[g], [bool(reach_g >> p & 1) for p in range(P)])
            if not (role[g, Lg] == LEADER and up[g] >> Lg & 1):
                Lg = -1
            fn, mark = sched[k] if k < len(sched) else (_all_up, False)
            if mark:
                marked[g] = max(Lg, 0)
            new_up, conn_g = fn(P, Lg, int(marked[g]), int(up[g]))
            if new_up == "bounce":
                to_crash += [g * P + p for p in range(P)]
                to_arm += [g * P + p for p in range(P)]
                c["bounce"] += 1
                new_up = full
            else:
                down, back = int(up[g]) & ~new_up, new_up & ~int(up[g])
                to_crash += [g * P + p for p in range(P) if down >> p & 1]
                to_arm += [g * P + p for p in range(P) if back >> p & 1]
                c["leader_crashed"] += int(Lg >= 0 and bool(down >> Lg & 1))
            up[g], conn_want[g] = new_up, conn_g
            phase_commit[g] = commit[g].max()
        if to_crash:
            crash(to_crash, f"P {P} tick {t}: crash")
            c["crashes"] += len(to_crash)
        if to_arm:
            arm(to_arm, t)
            c["restarts"] += len(to_arm)
        reach = (up & conn_want).astype(np.uint8)
        m.set_reachable(reach)
        if e is not None:
            e.set_reachable(reach)
        if to_crash or to_arm:
            both(f"P {P} tick {t}: after crash / restart")
        stt = m.state()
        if t % SCEN_START_EVERY == 0:                        # Start at every Leader, the cut-off ones too
            slots = np.nonzero(stt["state"] == LEADER)[0].astype(np.int32)
            if len(slots):
                b = m.o.start(slots, np.ones(len(slots), np.int32))
                if e is not None:
                    for x, y in zip(e.start(slots, np.ones(len(slots), np.int32)), b):
                        assert np.array_equal(x, y), (t, "start")
        conn = connected(reach, G, P)
        upb = connected(up.astype(np.uint8), G, P)
        before = {k: stt[k].copy() for k in STATE_FIELDS}
        ed0, hd0 = m.ed.copy(), m.hd.copy()
        want = m.clock_step(t, True)
        if e is not None:
            got = e.clock_step(t, True)
            for n in outs:
                assert np.array_equal(got[n], want[n]), (t, n, np.nonzero(got[n] != want[n])[0][:8])
            both(f"P {P} tick {t}")
        stt = m.state()
        role, term = stt["state"].reshape(G, P), stt["current_term"].reshape(G, P)
        # a replica that is down is bit-identical across the step, timers included
        dn = ~upb.reshape(-1)
        c["down_ticks"] += int(dn.sum())
        for k in STATE_FIELDS:
            a, b = stt[k], before[k]
            rows = G * P
            assert np.array_equal(a.reshape(rows, -1)[dn], b.reshape(rows, -1)[dn]), (t, k, "a down replica changed")
        assert np.array_equal(m.ed[dn], ed0[dn]) and np.array_equal(m.hd[dn], hd0[dn]), (t, "a down replica's timers")
        # at most one Leader per term; none elected without an up-and-connected majority
        for g, p in zip(*np.nonzero(role == LEADER)):
            assert leader_of_term[g].setdefault(int(term[g, p]), int(p)) == p, (g, "two Leaders in one term")
        new = (role == LEADER) & (before["state"].reshape(G, P) != LEADER)
        assert not (new & (conn.sum(axis=1) <= P // 2)[:, None]).any(), "a Leader elected without a majority"
        c["elected_after_crash"] += int((new & (up != full)[:, None]).sum())
        # the applier: engine and model agree; every applied Index carries one term per group, across
        # restarts (a restarted replica applies again from its dummy: the same terms)
        ofr, oto = m.o.collect_apply()
        has = oto >= ofr
        if e is not None:
            sl, fr, to, _ = e.collect_apply_compact()
            assert np.array_equal(sl, np.nonzero(has)[0]) and np.array_equal(fr, ofr[has]) and np.array_equal(to, oto[has])
        logs = logical_logs(stt, G, P, L)
        for s in np.nonzero(has)[0]:
            g = int(s) // P
            for i in range(int(ofr[s]), int(oto[s]) + 1):
                tm = int(logs[s, i - stt["dummy_index"][s]])
                assert applied[g].setdefault(i, tm) == tm, (g, i, "two replicas applied different entries")
                if i in applied_by[s]:
                    assert applied_by[s][i] == tm, (s, i, "a committed entry changed across a restart")
                    c["reapplied"] += 1
                applied_by[s][i] = tm
                c["agree"] += 1
    return c


def main():
    from multiraft_amd import Engine
    return run_all([(n,) for n in NAMES], lambda n: run_family(n, Engine), n_items)


if __name__ == "__main__":
    sys.exit(main())
