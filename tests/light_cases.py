"""States built group by group for the light tick (MRAFT_TICK_LIGHT,
include/mraft.h; k_tick_lite in multiraft_amd/csrc/mraft_tick_lite.hip). Test
infrastructure, numpy only.

Nothing here runs a workload forward: every group's leader log, every
follower's log, dummy, ring head, term, role, commitIndex and the leader's
nextIndex / matchIndex words are chosen, so the branch of the light launch a
group takes is known by construction. Each group carries the tag
`expect_listed`: whether the stated settle rule (every follower replies a
success that needs no compare, prevLogTerm matches, a heartbeat or an append
at the follower's last Index of at most LITE_SPAN entries that fits the ring,
commitIndex settling at log[last]) sends it to the full tick. `settle_rule`
restates that rule over the state arrays alone, so the tags can be checked
against it without the builder.

Terms: Index i of a group carries term TB + (i - leader dummy) unless a case
overrides it: strictly increasing, so a word copied to or from the wrong ring
slot changes the state. Dead ring slots hold POISON.

Families (see each function): A pure appends, B Start fused, C capacity
boundaries, D follower words, E a1's probe, F terms_sorted at the dummy."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from message_cases import shift_indices, top_offset
from oracle_lib import terms_sorted_exact

from multiraft_amd._abi import CANDIDATE, FOLLOWER, ITEM_BAD_SLOT, ITEM_LOG_FULL, LEADER
from multiraft_amd.engine import new_state

LITE_SPAN = 64  # kLiteSpan in multiraft_amd/csrc/mraft_tick_lite.hip: the longest run the light launch copies
CAPACITIES = (37, 64, 99, 256)
PEERS = (2, 3, 4, 5, 6, 7, 8)
FAMILIES = ("A", "B", "C", "D", "E", "F")
TB = 100       # term of a group's leader dummy
POISON = 7777  # dead ring slots
INDEX_TOP = 2**31 - 2  # the highest Index (include/mraft.h)
# what a settled group's tick leaves at a peer: a follower ends at the leader's last (PEER_APPEND), keeps its
# longer log (PEER_EXTRA: a heartbeat to a log that runs past prev), or is ahead of the leader's nextIndex and
# its reply is dropped (PEER_BELOW: nextIndex / matchIndex stay)
PEER_LEADER, PEER_APPEND, PEER_EXTRA, PEER_BELOW = 0, 1, 2, 3


@dataclass
class Case:
    name: str
    family: str
    P: int
    L: int
    state: dict
    leader_peer: np.ndarray
    counts: np.ndarray | None      # for start_and_tick; None: the case has no Start
    expect_listed: np.ndarray      # bool [G]
    start_expect: tuple | None     # Start's (index, term, is_leader, err) per group, as intended
    kinds: list                    # a short word per group: what it was built for
    peer_kind: np.ndarray          # [G, P]: PEER_LEADER, PEER_APPEND, PEER_EXTRA or PEER_BELOW

    @property
    def G(self) -> int:
        return len(self.leader_peer)

    @property
    def n_listed(self) -> int:
        return int(self.expect_listed.sum())

    @property
    def n_light(self) -> int:
        return self.G - self.n_listed


# ------------------------------------------------------------------ builder
def _fol(lag, fd=0, w=0, extra=(), term=None, voted=-1, role=FOLLOWER, commit=None, over=None, match=None,
         below=False):
    """One follower: it holds the group's entries from Index ldummy + fd up to
    prev = last0 - lag (the leader's nextIndex - 1), then `extra` terms past
    prev; `w`: how many entries of the run from prev + 1 fit before its ring
    wraps. below=True: compacted to its own last (dummy = last = prev + 1), so
    prev sits below its dummy."""
    return dict(lag=lag, fd=fd, w=w, extra=tuple(extra), term=term, voted=voted, role=role, commit=commit,
                over=over or {}, match=match, below=below)


def _mk(P, L, q, ldummy, m0, fols, kind, kcnt=0, lw=0, T=None, gover=None, c0=None, listed=False):
    """One group. The leader (peer q % P) holds Indexes ldummy .. last0 =
    ldummy + m0; `lw`: how many entries of the longest run to send fit before
    the leader's ring wraps; gover: {Index: term} overrides every replica
    sees; T: currentTerm (default: the term of last0, at least 1)."""
    assert len(fols) == P - 1 and 0 <= m0 <= L - 1
    gover = gover or {}
    last0 = ldummy + m0

    def tf(i):
        return gover.get(i, TB + (i - ldummy))

    T = tf(last0) if T is None else T
    run0 = min([last0 - f["lag"] + 1 for f in fols] + [last0 + 1])
    reps = []
    lp = q % P
    c0 = ldummy if c0 is None else c0
    leader = dict(dummy=ldummy, last=last0, head=(-lw - (run0 - ldummy)) % L,
                  terms=[tf(i) for i in range(ldummy, last0 + 1)], term=T, voted=lp, role=LEADER, commit=c0)
    nxt, mat, pk = [0] * P, [0] * P, [PEER_LEADER] * P
    it = iter(fols)
    for j in range(P):
        if j == lp:
            reps.append(leader)
            nxt[j], mat[j] = last0 + 1, last0
            continue
        f = next(it)
        prev = last0 - f["lag"]
        if f["below"]:
            fdummy = flast = prev + 1
            terms = [f["over"].get(fdummy, tf(fdummy))]
            head = f["w"] % L
        else:
            fdummy = ldummy + f["fd"]
            assert fdummy <= prev, (kind, fdummy, prev)
            flast = prev + len(f["extra"])
            terms = [f["over"].get(i, tf(i)) for i in range(fdummy, prev + 1)] + list(f["extra"])
            head = (-f["w"] - (prev + 1 - fdummy)) % L
        assert flast - fdummy <= L - 1, (kind, flast, fdummy)
        fc = f["commit"]
        reps.append(dict(dummy=fdummy, last=flast, head=head, terms=terms, term=T if f["term"] is None else f["term"],
                         voted=f["voted"], role=f["role"], commit=max(fdummy, min(c0, prev)) if fc is None else fc))
        nxt[j] = prev + 1
        pk[j] = PEER_BELOW if f["below"] else PEER_EXTRA if f["extra"] else PEER_APPEND
        mat[j] = max(0, prev) if f["match"] is None else f["match"]
    return dict(lp=lp, reps=reps, next=nxt, match=mat, kcnt=kcnt, listed=listed, kind=kind, T=T, last0=last0,
                m0=m0, pk=pk)


def _assemble(name, family, P, L, groups, use_counts, top=None):
    G = len(groups)
    st = new_state(G, P, L)
    log = st["log_term"].reshape(G * P, L)
    log[:] = POISON
    lp = np.zeros(G, np.int32)
    counts = np.zeros(G, np.int32)
    listed = np.zeros(G, bool)
    for g, gr in enumerate(groups):
        lp[g], counts[g], listed[g] = gr["lp"], gr["kcnt"], gr["listed"]
        for j, r in enumerate(gr["reps"]):
            s = g * P + j
            st["dummy_index"][s], st["last_index"][s], st["log_head"][s] = r["dummy"], r["last"], r["head"]
            st["current_term"][s], st["voted_for"][s], st["state"][s] = r["term"], r["voted"], r["role"]
            st["commit_index"][s] = r["commit"]
            log[s, (r["head"] + np.arange(len(r["terms"]))) % L] = r["terms"]
            # the other replicas' own rows (never read by this leader's tick): nextIndex as a new leader sets it
            if j == gr["lp"]:
                st["next_index"][s * P:(s + 1) * P] = gr["next"]
                st["match_index"][s * P:(s + 1) * P] = gr["match"]
            else:
                st["next_index"][s * P:(s + 1) * P] = r["last"] + 1
    st["last_applied"][:] = np.minimum(st["commit_index"], st["last_index"])
    off = 0
    if top is not None:  # the highest Index of the state at INDEX_TOP - top
        off = top_offset(st, top)
        st = shift_indices(st, off)
    st["terms_sorted"] = terms_sorted_exact(st, G, P, L)
    se = None
    if use_counts:
        idx, term = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
        isl, err = np.zeros(G, np.int32), np.zeros(G, np.int32)
        for g, gr in enumerate(groups):
            k = gr["kcnt"]
            if k < 0:
                err[g] = ITEM_BAD_SLOT
            elif k > 0:
                last0 = gr["last0"] + off
                if gr["m0"] + k > L - 1 or last0 + k > INDEX_TOP:
                    err[g] = ITEM_LOG_FULL
                else:
                    idx[g], term[g], isl[g] = last0 + 1, gr["T"], 1
        se = (idx, term, isl, err)
    return Case(name, family, P, L, st, lp, counts if use_counts else None, listed, se, [gr["kind"] for gr in groups],
                np.array([gr["pk"] for gr in groups], np.int32).reshape(G, P))


def _spread(lag_main, lags, w, nf, wmul=3):
    """P - 1 followers as (lag, wrap offset): one (w % nf) lags by lag_main, the
    others by smaller members of `lags`; each one's ring wraps at its own
    offset of its run."""
    le = [x for x in lags if x <= lag_main]
    # over the groups w = 0 .. lag_main - 1 the slowest follower's offset a * w + 1 (a coprime to the span)
    # takes every value once, in another order than the leader's w
    a = next(x for x in (5, 7, 11, 3, 1) if np.gcd(x, max(lag_main, 1)) == 1)
    out = []
    for i in range(nf):
        if i == w % nf:
            out.append((lag_main, (a * w + 1) % max(lag_main, 1)))
        else:
            lag = le[(w + i) % len(le)]
            out.append((lag, (w + 1 + wmul * i) % max(lag, 1)))
    return out


# ---------------------------------------------------------------- family A
A_SPANS = (1, 3, 4, 5, 7, 8, 9, 12, 63, 64)


def _groups_a(P, L, light_only):
    """Pure appends: per span n, n groups whose leader ring wraps after
    0 .. n-1 entries of the copied run, each follower's ring at another
    offset; the other followers lag by smaller spans. n = 65: listed."""
    nf, out = P - 1, []
    for n in A_SPANS + (() if light_only else (LITE_SPAN + 1,)):
        if n > L - 1:
            continue
        for w in (range(n) if n <= LITE_SPAN else (0, 1, 7, 33, 64)):
            keep = min((w + n) % 3, L - 1 - n)  # entries the slowest follower already holds
            m0 = n + keep
            fols = []
            for i, (lag, fw) in enumerate(_spread(n, A_SPANS, w, nf)):
                fd = 0
                if lag < n and i % 3 == 1:
                    fd = min(1, m0 - lag)             # a dummy above the leader's
                elif i % 3 == 2 and m0 + 1 <= L - 1:
                    fd = -1                           # ... and below it
                fols.append(_fol(lag, fd=fd, w=fw))
            c0 = 5 + w % 4 + max(0, keep - w % 2)
            out.append(_mk(P, L, w + n, 5 + w % 4, m0, fols, f"n{n}", lw=w, c0=c0, listed=n > LITE_SPAN))
    return out


# ---------------------------------------------------------------- family B
B_COUNTS = (1, 4, 5, 6, 17, 60, 64)
B_LAGS = (0, 1, 2, 3, 5, 6)


def _groups_b(P, L, light_only):
    """Start fused: kcnt new entries (currentTerm, never loaded) behind `lag`
    entries loaded from the leader's log, the boundary at every position of a
    group of four; nextIndex = last0 + 2 (prev is an entry Start appends);
    a pre-Start log[last0] above currentTerm (Start clears terms_sorted)."""
    nf, out = P - 1, []
    for kc in B_COUNTS:
        for lag in B_LAGS:
            n = lag + kc
            keep = (kc + lag) % 3
            if lag + keep + kc > L - 1:
                keep = 0
            if n > LITE_SPAN or lag + kc > L - 1:
                continue
            m0 = lag + keep
            for w in sorted({0, 1, lag, lag + 1, n // 2, n - 1} & set(range(n))):
                fols = [_fol(lg, w=(w + 1 + 3 * i) % (lg + kc)) for i, (lg, _) in
                        enumerate(_spread(lag, B_LAGS, w, nf))]
                ld = 3 + w % 5
                out.append(_mk(P, L, w + kc + lag, ld, m0, fols, f"k{kc}lag{lag}", kcnt=kc, lw=w,
                               T=TB + m0 + w % 2, c0=ld + keep))
    for kc in (1, 2, 5, 6):      # nextIndex = last0 + 2: prev = last0 + 1 is Start's first entry
        for m0 in (0, 2):
            if m0 + kc > L - 1:
                continue
            for same in (True,) if light_only else (True, False):
                T = TB + m0 + 2
                for w in range(min(kc, 3)):
                    fols = [_fol(-1 if i == w % nf else 0, w=w, over={3 + m0 + 1: T if same else T - 1})
                            for i in range(nf)]
                    out.append(_mk(P, L, w + kc, 3, m0, fols, f"next+2k{kc}", kcnt=kc, lw=(w + 1) % kc, T=T, c0=3,
                                   listed=not same))
    for kc in (1, 5):            # log[last0] above currentTerm, last0 > dummy
        for lag in (0, 1):
            for w in range(2):
                m0 = 3 + lag
                fols = [_fol(lag if i == w % nf else 0, w=w) for i in range(nf)]
                out.append(_mk(P, L, w + kc + lag, 4, m0, fols, "lastAboveT", kcnt=kc, lw=w, T=TB + m0,
                               gover={4 + m0: TB + m0 + 3}, c0=4 + 1))
    return out


# ---------------------------------------------------------------- family C
def _groups_c(P, L, light_only):
    """Capacity: a follower whose dummy is below the leader's ends at
    last - fdummy = L - 1 (light) or L (listed); Start fills the leader's ring
    to last0 + kcnt - ldummy = L - 1 (appends) or L (MRAFT_ITEM_LOG_FULL: no
    entry, the tick still runs)."""
    nf, out = P - 1, []
    for d in (1, 3):
        for lag in (1, 5):
            for kc in (0, 2):
                for over in (0,) if light_only else (0, 1):
                    m0 = L - 1 - d - kc + over
                    for w in (0, lag + kc - 1):
                        fols = [_fol(lag, fd=-d if i == w % nf else 0, w=(w + i) % (lag + kc)) for i in range(nf)]
                        out.append(_mk(P, L, w + d + lag, 9, m0, fols, f"fcap{'+1' if over else ''}", kcnt=kc, lw=w,
                                       T=TB + m0, c0=9 + m0 - lag, listed=bool(over)))
    for kc in (1, 5, LITE_SPAN):
        if kc > L - 2:
            continue
        for lag in (0, 2):
            if lag + kc > LITE_SPAN:
                continue
            for full in (0, 1):
                m0 = L - 1 - kc + full
                for w in (0, kc - 1):
                    fols = [_fol(lag if i == w % nf else 0, w=(w + i) % kc) for i in range(nf)]
                    out.append(_mk(P, L, w + kc + lag, 2, m0, fols, "ringfull" if full else "ringfits", kcnt=kc,
                                   lw=w, T=TB + m0 + 1, c0=2 + m0 - lag))
    return out


def _groups_c_top(P, L, J):
    """Every leader's last0 is the state's highest Index, moved to INDEX_TOP -
    J: Start of J entries ends at INDEX_TOP (appends), J + 1 one above it
    (MRAFT_ITEM_LOG_FULL by the Index domain, the ring has room), and a ring
    filled to L with J entries at the top of the domain too."""
    nf, out = P - 1, []
    K0 = 400
    for kc in (J, J + 1):
        for lag in (0, 1, 2, 3):
            for w in range(2):
                m0 = lag + 1 + w
                fols = [_fol(lag if i == w % nf else 0, w=w) for i in range(nf)]
                out.append(_mk(P, L, w + lag, K0 - m0, m0, fols, "topfits" if kc == J else "topfull", kcnt=kc,
                               lw=(w + lag) % (lag + kc), T=TB + m0, c0=K0 - lag))
    for w in range(2):
        m0 = L - J
        fols = [_fol(1 if i == w % nf else 0, w=w) for i in range(nf)]
        out.append(_mk(P, L, w, K0 - m0, m0, fols, "topringfull", kcnt=J, lw=w, T=TB + m0, c0=K0 - 1))
    return out


# ---------------------------------------------------------------- family D
def _groups_d(P, L, light_only):
    """The follower's own words: term below / equal with votedFor set, role
    candidate or leader, commitIndex below / at / above the leader's; a
    leader commitIndex above the follower's new last on a heartbeat; a
    heartbeat to a follower whose log runs past prev. Listed: a follower of a
    higher term (stale leader), a prevLogTerm mismatch on a heartbeat."""
    nf, out = P - 1, []
    q = 0
    for n in (0, 2, 6):
        for dt in (0, -1, -3):
            for voted in (-1, 0, P - 1):
                for role in (FOLLOWER, CANDIDATE, LEADER):
                    m0 = 8 + n
                    ld = 6 + q % 3
                    c0 = ld + 4
                    fc = c0 + (-2, 0, 1)[q % 3]
                    fols = [_fol(n, w=q % max(n, 1), term=TB + m0 + dt, voted=voted, role=role, commit=fc)
                            if i == q % nf else _fol(n if i % 2 else 0, w=i % max(n, 1)) for i in range(nf)]
                    out.append(_mk(P, L, q, ld, m0, fols, f"words n{n}", lw=q % max(n, 1), c0=c0))
                    q += 1
    for q in range(12):  # heartbeats: the leader's commitIndex above its last, followers running past prev
        m0, ld = 5, 4
        extra = (TB + m0,) * (q % 3)
        c0 = ld + m0 + (q // 3) % 2 + (q // 6)
        fols = [_fol(0, w=i, extra=extra if i == q % nf else (), commit=ld + m0 - (q + i) % 3, term=TB + m0 - i % 2,
                     voted=i % P) for i in range(nf)]
        out.append(_mk(P, L, q, ld, m0, fols, "hb c0/extra", c0=c0))
    if not light_only:
        for q in range(8):
            n, m0, ld = (0, 3)[q % 2], 7, 5
            if q < 4:   # the follower's term above the leader's
                fols = [_fol(n, w=i, term=TB + m0 + (1 if i == q % nf else 0)) for i in range(nf)]
                kind = "stale"
            else:       # another term at prev
                fols = [_fol(n, w=i, over={ld + m0 - n: TB + 1} if i == q % nf else None) for i in range(nf)]
                kind = "prevmismatch"
            out.append(_mk(P, L, q, ld, m0, fols, kind, lw=q % 3, c0=ld + 2, listed=True))
    return out


# ---------------------------------------------------------------- family E
def _groups_e(P, L, light_only):
    """a1's probe of log[last]: currentTerm (commitIndex advances), below it
    under terms_sorted (no advance, settles), below it without terms_sorted
    (a scan: listed), last == commitIndex; for P >= 4 groups with fewer than
    P/2 successes whose appended span is 5 .. 64."""
    nf, out = P - 1, []
    q = 0
    for n in (0, 1, 6):
        for srt in (True, False):
            for dT in (0, 2):
                for atc in (False, True):    # commitIndex == last
                    m0, ld = 7 + n, 3 + q % 4
                    gover = None if srt else {ld + 1: TB + 4}   # Index dummy+1 above dummy+2: not sorted
                    listed = (not srt) and dT > 0 and not atc
                    if listed and light_only:
                        continue
                    fols = [_fol(n if i == q % nf else (n // 2), w=(q + i) % max(n, 1)) for i in range(nf)]
                    out.append(_mk(P, L, q, ld, m0, fols, f"probe n{n} srt{int(srt)} dT{dT} atc{int(atc)}",
                                   lw=q % max(n, 1), T=TB + m0 + dT, gover=gover,
                                   c0=ld + m0 if atc else ld + 2, listed=listed))
                    q += 1
    if P >= 4:
        for span in (5, 9, 33, LITE_SPAN):
            if span + 4 > L - 1:
                continue
            for var in ("top", "low", "scan", "lowered"):
                if light_only and var in ("scan", "lowered"):
                    continue
                for nsucc in range(1, P // 2):
                    for w in (0, 3, span - 1):
                        m0, ld = span + 4, 7
                        last0, c0 = ld + m0, ld + 2
                        srt, dT = var != "scan", 2 if var == "scan" else 0
                        gover = None if srt else {ld + 1: TB + 4}
                        am = {"top": last0, "low": c0 - w % 2, "scan": last0 - 1, "lowered": last0}[var]
                        fols = []
                        for i in range(nf):
                            if i < nsucc:
                                fols.append(_fol(span, w=(w + i) % span,
                                                 match=last0 + 2 if var == "lowered" and i == 0 else None))
                            else:   # ahead of the leader's nextIndex: prev below its dummy, the reply dropped
                                fols.append(_fol(1 + (i + w) % 3, w=i + w, below=True, match=am,
                                                 commit=last0 - (1 + (i + w) % 3) + 1))
                        out.append(_mk(P, L, w + nsucc, ld, m0, fols, f"few {var} s{span}", lw=w, T=TB + m0 + dT,
                                       gover=gover, c0=c0, listed=var in ("scan", "lowered")))
    return out


# ---------------------------------------------------------------- family F
def _groups_f(P, L, light_only):
    """prev == the leader's dummy: the term at the dummy below, equal to and
    above the first appended entry's; the follower's dummy equal to prev and
    below it; the first entry loaded from the log or appended by Start.
    Listed: the follower's term at prev differs."""
    nf, out = P - 1, []
    q = 0
    for n in (1, 3, 6):
        for dterm in (TB, TB + 1, TB + 9):      # the first entry's term is TB + 1
            for fd in (0, -2):
                for kc in (0, 5):
                    for bad in (False,) if light_only else (False, True):
                        ld = 8
                        m0 = n if kc == 0 else 0     # Start appends the whole run
                        T = TB + max(m0, 1)
                        fols = [_fol(m0, fd=fd if i == q % nf else 0, w=(q + i) % (m0 + kc),
                                     over={ld: TB + 2} if bad and i == q % nf else None) for i in range(nf)]
                        out.append(_mk(P, L, q, ld, m0, fols, f"dummy n{n} t{dterm - TB} fd{fd} k{kc}", kcnt=kc,
                                       lw=q % (m0 + kc), T=T, gover={ld: dterm}, c0=ld, listed=bad))
                        q += 1
    return out


_BUILD = {"A": (_groups_a, False), "B": (_groups_b, True), "C": (_groups_c, True), "D": (_groups_d, False),
          "E": (_groups_e, False), "F": (_groups_f, True)}


@functools.lru_cache(maxsize=8)
def cases(family: str, P: int, L: int) -> tuple:
    """The family's cases at (P, L): `<family>-mixed` (light and listed
    groups), `<family>-light` (the light-tagged groups only: 0 fallbacks), and
    for C the top of the Index domain. Treat the states as read-only."""
    fn, use_counts = _BUILD[family]
    out = [_assemble(f"{family}-mixed", family, P, L, fn(P, L, False), use_counts),
           _assemble(f"{family}-light", family, P, L, fn(P, L, True), use_counts)]
    if family == "C":
        J = 1 + 2 * (P % 3)
        out.append(_assemble("C-top-light", family, P, L, _groups_c_top(P, L, J), True, top=J))
    return tuple(out)


CASE_NAMES = tuple(f"{f}-{v}" for f in FAMILIES for v in ("mixed", "light")) + ("C-top-light",)


def case(name: str, P: int, L: int) -> Case:
    for c in cases(name[0], P, L):
        if c.name == name:
            return c
    raise KeyError(name)


def tiny_cases(G: int, P: int, L: int = 99):
    """Family A cut (or cycled) to exactly G groups: every group light-tagged,
    and every group listed (n = 65)."""
    light = _groups_a(P, L, True)
    light = [light[(i * 7) % len(light)] for i in range(G)]
    listed = [g for g in _groups_a(P, L, False) if g["listed"]]
    listed = [listed[i % len(listed)] for i in range(G)]
    return (_assemble(f"tiny-light-G{G}", "A", P, L, light, False),
            _assemble(f"tiny-listed-G{G}", "A", P, L, listed, False))


def bad_slot_case(P: int, L: int = 37):
    """counts = -1 under leader_peer -1 (idle: no error), in range
    (MRAFT_ITEM_BAD_SLOT, the tick runs) and P (MRAFT_ITEM_BAD_SLOT), beside
    groups that really Start. Returns (case, expected err)."""
    groups = []
    for q in range(12):
        fols = [_fol(1, w=0) for _ in range(P - 1)]
        groups.append(_mk(P, L, q, 2, 4, fols, "badslot", kcnt=-1 if q % 4 < 3 else 2, c0=3))
    c = _assemble("bad-slot", "B", P, L, groups, True)
    for g in range(len(groups)):
        if g % 4 == 0:
            c.leader_peer[g] = -1
            c.start_expect[3][g] = 0
        elif g % 4 == 1:
            c.leader_peer[g] = P
    return c


# ------------------------------------------------------ the rule, restated
def settle_rule(st: dict, P: int, L: int, lp: np.ndarray, counts: np.ndarray | None) -> np.ndarray:
    """Per group: True where the light launch's stated rule sends the group to
    the full tick, False where it settles it (or has nothing to do: an idle
    or non-leader group). From the state arrays alone."""
    G = len(lp)
    log = st["log_term"].reshape(G * P, L).astype(np.int64)
    out = np.zeros(G, bool)

    def term_at(s, i):
        return int(log[s, (int(st["log_head"][s]) + i - int(st["dummy_index"][s])) % L])

    for g in range(G):
        if not 0 <= lp[g] < P:
            continue
        ld = g * P + int(lp[g])
        T, c0 = int(st["current_term"][ld]), int(st["commit_index"][ld])
        last0, ldummy = int(st["last_index"][ld]), int(st["dummy_index"][ld])
        if st["state"][ld] != LEADER or c0 < ldummy:
            continue
        k = 0 if counts is None else int(counts[g])
        started = k > 0 and last0 + k - ldummy <= L - 1 and last0 + k <= INDEX_TOP
        last = last0 + k if started else last0

        def lterm(i):
            return T if i > last0 else term_at(ld, i)

        srt = bool(st["terms_sorted"][ld]) and not (started and last0 > ldummy and term_at(ld, last0) > T)
        listed, nsucc, words, lowered = False, 0, [], False
        for j in range(P):
            if j == lp[g]:
                continue
            f = g * P + j
            prev = int(st["next_index"][ld * P + j]) - 1
            n = last - prev
            ft, fdummy, flast = int(st["current_term"][f]), int(st["dummy_index"][f]), int(st["last_index"][f])
            old = int(st["match_index"][ld * P + j])
            if prev < ldummy or prev > last or T < ft:     # snapshot, panic, stale
                listed = True
            elif prev < fdummy:                             # below the follower's dummy: reply dropped (T > 0)
                listed |= T <= 0
                words.append(old)
            elif prev > flast or (n > 0 and (flast != prev or n > LITE_SPAN or last - fdummy > L - 1)):
                listed = True
            elif term_at(f, prev) != lterm(prev):           # prevLogTerm
                listed = True
            else:
                nsucc += 1
                lowered |= old > last
                words.append(max(old, last))
        if listed or nsucc == 0:
            out[g] = listed
            continue
        if nsucc >= P // 2:
            top = last
        else:  # few successes: the (P/2)-th largest word bounds every evaluation's top
            top = min(sorted(words, reverse=True)[P // 2 - 1], last)
            if top > c0 and lowered:
                out[g] = True
                continue
        if top > c0:
            t = lterm(top)
            out[g] = not (t == T or (srt and t < T))
    return out


def oracle_start_and_tick(o, lp, counts, G: int, P: int):
    """mraft_start on the oracle over the leader slots of the groups whose
    counts are set (leader_peer in range), then its tick: what
    mraft_start_and_tick must equal. Returns (group flags, Start's outputs)."""
    idx, term = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    isl, err = np.zeros(G, np.int32), np.zeros(G, np.int32)
    sel = np.flatnonzero((lp >= 0) & (lp < P) & (counts != 0))
    if len(sel):
        oi, ot, ol, oe = o.start((sel * P + lp[sel]).astype(np.int32), counts[sel].astype(np.int32))
        idx[sel], term[sel], isl[sel], err[sel] = oi, ot, ol, oe
    err[(lp >= P) & (counts != 0)] = ITEM_BAD_SLOT
    return o.replicate_tick(lp), (idx, term, isl, err)
