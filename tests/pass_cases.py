"""States built group by group for the streaming merge pass
(multiraft_amd/csrc/mraft_pass.h: pass_pipe, pass_chunk, copy_loop) and the
downward scans beside it (mraft_device.h: wave_scan_down_ne /
wave_conflict_scan, wave_scan_down_eq). Test infrastructure, numpy only, in
the style of tests/light_cases.py.

Every group's leader log, every follower's log, dummy, ring head, term, role,
commitIndex and the leader's nextIndex / matchIndex words are chosen, so where
each decision of the pass falls on its chunk grid is known by construction.
Each group carries a `kind` string and, per follower, the intended outcome
(reply class, first Index written or None, resulting last Index, ConflictIndex
or None). `geometry` restates the pass's grid rules over the state arrays
alone (it never sees the builder's inputs), so tests/test_pass_cases.py can
check that every cell a family claims is really there.

Terms: Index i of a group carries term TB + (i - leader dummy) unless a case
overrides it: strictly increasing, so a word copied to or from the wrong ring
slot changes the state. Dead ring slots hold POISON (the `tail` kind excepted:
there they hold the leader's terms, so a compare that runs past the follower's
end sees no mismatch).

Forms (the dispatcher's choice, mraft_tick_body.inc / handle_one):
  vec    dwordx4: L % 4 == 0, rows aligned alike, log 16-B aligned
  mis1-3 dword: the follower's head - dummy differs from the leader's by 1, 2, 3 mod 4
  odd    dword: L = 1023
  bound  dword: rows aligned alike at L = 1024, for log_term bound 4, 8 or 12 B past a 16-B boundary

Families: M one merging follower (forms vec, mis1, odd), W ring wraps, F the forms, N several
followers in one pass, S the commit scan riding the pass, C ConflictIndex
scans, D one descent in the shipped entries (message path), V entries by value
at chosen buffer layouts (`value_layout` over the V and N states)."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle_lib import terms_sorted_exact

from multiraft_amd._abi import FOLLOWER, LEADER
from multiraft_amd.engine import entry_positions, new_state

CHUNK = 256   # entries per chunk of the pass (mraft_pass.h: CW = 64 * EPL, EPL = 4; pass_chunk<1>: 256 * V)
LINE = 32     # entries per 128-B line: MRAFT_TICK_ALIGN (mraft_tick.hip), handle_one's `& 31` (mraft_handle_ae.h)
WAVE = 64     # lanes; the ConflictIndex probe reads one term per lane
TB = 5000     # term of a group's leader dummy
POISON = 7777
FORMS = ("vec", "mis1", "mis2", "mis3", "odd", "bound")

OFFS = (0, 1, 3, 4, 28, 31)
RELS = ("first", 1, 3, 4, 251, 252, 255, 256, 257, 259, 260, 511, 512)
# the dword forms' lane is rel % 64 and its entry (rel % 256) // 64: both sides of every 64-entry edge as well
RELS_DWORD = RELS + (63, 64, 127, 128, 191, 192)
KINDS = ("mismatch", "beyond", "match_longer", "tail")
NENDS = ("m+1", "m+2", "m+5", "E", "E+1", "E+256", "E+257", "E+259")
C_RUNS = (0, 1, 62, 63, 64, 65, 127, 128, 129, 319, 320, 321, 600)
C_BREAKERS = (2, 3, "absent")
S_FULL_LENS = (1, 63, 64, 65, 255, 256, 257, 513)


def form_L(form: str) -> int:
    return 1023 if form == "odd" else 1024


def form_mis(form: str) -> int:
    return int(form[3]) if form.startswith("mis") else 0


@dataclass
class Case:
    name: str
    family: str
    form: str
    P: int
    L: int
    state: dict
    leader_peer: np.ndarray
    kinds: list          # a short string per group
    expect: list         # per group {peer: (class, first Index written or None, resulting last, ConflictIndex or None)}
    rejected: np.ndarray  # bool [G]: built to be rejected (G_LOG_FULL / ITEM_LOG_FULL at some follower)

    @property
    def G(self) -> int:
        return len(self.leader_peer)


# ------------------------------------------------------------------ builder
def _f(prev, last, dummy, expect, wrap=None, over=None, dead=None, term=None, voted=-1, role=FOLLOWER, commit=None,
       match=None):
    """One follower: it holds Indexes dummy .. last (the group's terms unless
    `over` {Index: term} says otherwise); the leader's nextIndex for it is
    prev + 1; `wrap`: the Index that sits at ring slot 0 (default: its dummy);
    `dead` {Index: term}: words left in dead ring slots."""
    return dict(prev=prev, last=last, dummy=dummy, expect=expect, wrap=wrap, over=over or {}, dead=dead or {},
                term=term, voted=voted, role=role, commit=commit, match=match)


def _group(P, L, lp, ldummy, llast, lwrap, fols, kind, T=None, c0=None, gover=None, rejected=False):
    """One group. The leader (peer lp) holds Indexes ldummy .. llast, Index
    lwrap at ring slot 0; gover: {Index: term} overrides every replica sees;
    T: currentTerm (default: the term of llast)."""
    assert len(fols) == P - 1 and 0 <= llast - ldummy <= L - 1, kind
    gover = gover or {}

    def tf(i):
        return gover.get(i, TB + (i - ldummy))

    T = tf(llast) if T is None else T
    c0 = ldummy if c0 is None else c0
    assert ldummy <= c0 <= llast, kind
    reps, nxt, mat, expect = [], [0] * P, [0] * P, {}
    it = iter(fols)
    for j in range(P):
        if j == lp:
            reps.append(dict(dummy=ldummy, last=llast, head=(ldummy - lwrap) % L,
                             terms=[tf(i) for i in range(ldummy, llast + 1)], dead={}, term=T, voted=lp, role=LEADER,
                             commit=c0))
            nxt[j], mat[j] = llast + 1, llast
            continue
        f = next(it)
        fd, fl = f["dummy"], f["last"]
        assert 0 <= fl - fd <= L - 1 and fd >= 0, (kind, fd, fl)
        assert all(fl < i < fd + L for i in f["dead"]), kind
        wrap = fd if f["wrap"] is None else f["wrap"]
        fc = f["commit"]
        fc = min(max(fd, min(c0, f["prev"])), fl) if fc is None else fc
        reps.append(dict(dummy=fd, last=fl, head=(fd - wrap) % L, terms=[f["over"].get(i, tf(i)) for i in range(fd, fl + 1)],
                         dead=f["dead"], term=T if f["term"] is None else f["term"], voted=f["voted"], role=f["role"],
                         commit=fc))
        nxt[j] = f["prev"] + 1
        mat[j] = max(0, min(f["prev"], llast)) if f["match"] is None else f["match"]
        expect[j] = f["expect"]
    return dict(lp=lp, reps=reps, next=nxt, match=mat, kind=kind, expect=expect, rejected=rejected)


def _assemble(name, family, form, P, L, groups):
    G = len(groups)
    st = new_state(G, P, L)
    log = st["log_term"].reshape(G * P, L)
    log[:] = POISON
    lp = np.zeros(G, np.int32)
    for g, gr in enumerate(groups):
        lp[g] = gr["lp"]
        for j, r in enumerate(gr["reps"]):
            s = g * P + j
            st["dummy_index"][s], st["last_index"][s], st["log_head"][s] = r["dummy"], r["last"], r["head"]
            st["current_term"][s], st["voted_for"][s], st["state"][s] = r["term"], r["voted"], r["role"]
            st["commit_index"][s] = r["commit"]
            for i, t in r["dead"].items():
                log[s, (r["head"] + i - r["dummy"]) % L] = t
            log[s, (r["head"] + np.arange(len(r["terms"]))) % L] = r["terms"]
            if j == gr["lp"]:
                st["next_index"][s * P:(s + 1) * P] = gr["next"]
                st["match_index"][s * P:(s + 1) * P] = gr["match"]
            else:   # the other replicas' own rows (never read by this leader's tick)
                st["next_index"][s * P:(s + 1) * P] = r["last"] + 1
    st["last_applied"][:] = np.minimum(st["commit_index"], st["last_index"])
    st["terms_sorted"] = terms_sorted_exact(st, G, P, L)
    return Case(name, family, form, P, L, st, lp, [gr["kind"] for gr in groups], [gr["expect"] for gr in groups],
                np.array([gr["rejected"] for gr in groups], bool))


# ---------------------------------------------------------------- family M
def _m_group(form, off, rel, kind, nv, fit, q, lw=None, fw=None, P=2):
    """One merging follower. `off`: where plo sits in its 128-B line of the
    leader's row; `rel`: the decision point m relative to the chunk origin
    (dwordx4 form: plo - off; dword forms: plo) or "first" (m = plo); `nv`:
    index into NENDS; lw / fw: the leader's / follower's ring wraps `lw`
    entries past the origin (None: not inside the range). None where the
    combination cannot exist (rel < off in the dwordx4 form, capacity)."""
    L, mis = form_L(form), form_mis(form)
    vec = form == "vec"
    gap = 1 + q % 3
    ldummy = 1100 + q % 7
    prev = ldummy + gap
    plo = prev + 1
    origin = plo - off if vec else plo
    if rel == "first":
        m = plo
    else:
        m = origin + rel
        if m < plo:
            return None
    E = origin + CHUNK * ((m - origin) // CHUNK + 1)   # the end of m's chunk
    nend = (m + 1, m + 2, m + 5, E, E + 1, E + CHUNK, E + CHUNK + 1, E + CHUNK + 3)[nv]
    if kind == "match_longer":
        nend = m + 1   # the compared range ends with the entries: the axis moves to the follower's excess
    llast = nend - 1
    if llast - ldummy > L - 1 or llast < m:
        return None
    # rings: Index `wrap` at slot 0. dwordx4 form: the leader's slot of plo is `off` mod 32 (L % 32 == 0 and
    # ld * L % 32 == 0 at L = 1024), the follower's wrap equal to the leader's mod 4 (plus `mis`)
    base = plo - off                                    # dword forms: plo's slot still `off` mod 32
    far = base - LINE if nend - base <= L - LINE else base
    lwrap = far if lw is None else origin + lw
    fwrap = far if fw is None else origin + fw
    if mis:   # head - dummy = -wrap (mod L): the follower's wrap `mis` below the leader's, mod 4
        if fw is None:
            fwrap -= (fwrap - lwrap) % 4
        elif lw is None:
            lwrap -= (lwrap - fwrap) % 4
        fwrap -= mis

    def tf(i):
        return TB + (i - ldummy)

    over, dead = {}, {}
    if kind == "mismatch":
        flast = (m, m + 2, llast + 3)[q % 3]
        if fit != "normal":
            flast = min(flast, llast - (fit == "over"))
            if flast < m:
                return None
        diverge = range(m, flast + 1) if q % 2 else (m,)
        over = {i: tf(i) + 20000 for i in diverge}
        over.update({i: tf(i) + 20000 for i in range(llast + 1, flast + 1)})
        exp = ("merge", m, llast, None)
    elif kind in ("beyond", "tail"):
        flast = m - 1
        exp = ("merge", m, llast, None)
    else:
        excess = (0, 1, 4, E - nend, E - nend + 1, 2, 5, 7)[nv]
        flast = llast + excess
        over = {i: tf(llast) for i in range(llast + 1, flast + 1)}
        exp = ("merge", None, flast, None)
        if fit != "normal":
            return None
    if fit == "normal":
        fdummy = ldummy + (0, 1 if prev > ldummy + 1 else 0, -1)[q % 3]
    elif fit == "exact":
        fdummy = llast - (L - 1)
    else:
        fdummy = llast - L
        exp = ("full", None, flast, None)
    if flast - fdummy > L - 1 or fdummy < 0 or fdummy > prev:
        return None
    if kind == "tail":   # dead slots past the follower's end repeat the leader's entries
        dead = {i: tf(i) for i in range(flast + 1, min(llast, fdummy + L - 1) + 1)}
    fol = _f(prev, flast, fdummy, exp, wrap=fwrap, over=over, dead=dead)
    c0 = ldummy + q % (gap + 1)
    fols = [fol] + [_f(llast, llast, ldummy, ("hb", None, llast, None), wrap=fwrap) for _ in range(P - 2)]
    return _group(P, L, q % P, ldummy, llast, lwrap, fols, f"{kind}/{fit}", c0=c0, rejected=fit == "over")


def _thin(offs, rels, nvs, build):
    """Pairwise coverage of (off, rel, nend): every pair of values of two
    axes with the third rotated until the combination can be built."""
    out, seen = [], set()

    def add(pick):
        for r in range(max(len(offs), len(rels), len(nvs))):
            o, l, n = pick(r)
            if (o, l, n) in seen:
                return
            g = build(o, l, n, len(out))
            if g is not None:
                seen.add((o, l, n))
                out.append(g)
                return

    for io, o in enumerate(offs):
        for il, l in enumerate(rels):
            add(lambda r: (o, l, nvs[(io + il + r) % len(nvs)]))
    for il, l in enumerate(rels):
        for n in nvs:
            add(lambda r: (offs[(il + n + r) % len(offs)], l, n))
    for io, o in enumerate(offs):
        for n in nvs:
            add(lambda r: (o, rels[(io + n + r) % len(rels)], n))
    return out


def m_rels(form):
    return RELS if form == "vec" else RELS_DWORD


def _groups_m(form, offs=OFFS, rels=None, nvs=tuple(range(len(NENDS)))):
    rels = m_rels(form) if rels is None else rels
    out = []
    for kind in KINDS:
        out += _thin(offs, rels, nvs, lambda o, l, n, q: _m_group(form, o, l, kind, n, "normal", q))
        if kind != "match_longer":
            for fit in ("exact", "over"):
                for io, o in enumerate(offs):
                    for il, l in enumerate(rels):
                        for r in range(len(nvs)):
                            g = _m_group(form, o, l, kind, nvs[(io + il + r) % len(nvs)], fit, len(out))
                            if g is not None:
                                out.append(g)
                                break
    return out


# ---------------------------------------------------------------- family F
F_OFFS, F_RELS = (0, 3, 28), ("first", 3, 255, 256, 260, 512)


def _groups_f(form):
    """The reduced M set, in the given form."""
    return _groups_m(form, F_OFFS, F_RELS)


# ---------------------------------------------------------------- family V
V_OFFS, V_RELS = (0, 1, 2, 3, 30), ("first", 3, 255, 256, 260)


def _groups_v(form):
    """The states family V's buffer layouts (value_layout) are laid over: a
    reduced M set whose followers' rows start at every phase mod 4."""
    return _groups_m(form, V_OFFS, V_RELS)


# ---------------------------------------------------------------- family W
W_OFFS, W_RELS = (0, 3, 28), ("first", 3, 255, 257, 511)
W_RELS_LONGER = (257, 511)
W_EDGE = CHUNK         # the wrap exactly at the first chunk's end
W_MID_VEC = (96, 100)  # mid-chunk: the leader's (a multiple of 32 in the dwordx4 form) and the follower's (of 4)


def w_wraps(form):
    """(leader wrap, follower wrap) pairs, entries past the origin; None: not
    in range. dwordx4 form: none / chunk edge / mid-chunk, independently; dword
    forms whose form does not depend on where the rings wrap (odd, bound):
    the mid-chunk wrap at every residue mod 4 as well."""
    if form == "vec" or form.startswith("mis"):
        # mis1-3: the dwordx4 form's pairs with the follower's wrap moved down by the misalignment (the form
        # is set by where the two rings wrap relative to each other)
        lws, fws = (None, W_EDGE, W_MID_VEC[0]), (None, W_EDGE, W_MID_VEC[1])
        return [(a, None if b is None else b - form_mis(form)) for a in lws for b in fws if (a, b) != (None, None)]
    ws = (W_EDGE, 100, 101, 102, 103)
    return [(w, None) for w in ws] + [(None, w) for w in ws] + [(w, ws[(i + 1) % len(ws)]) for i, w in enumerate(ws)] \
        + [(w, w) for w in ws]


def _groups_w(form):
    """The reduced M set with the rings' wraps inside the range: the entries
    always run a whole chunk past the decision point's chunk (NENDS E+256 ..)."""
    out = []
    for lw, fw in w_wraps(form):
        fw = None if fw is None else fw + form_mis(form)   # (_m_group moves it down again)
        for kind in KINDS:
            for io, o in enumerate(W_OFFS):
                for il, l in enumerate(W_RELS):
                    if kind == "match_longer" and l not in W_RELS_LONGER:
                        continue    # its entries end at m: only there do they reach past the wraps
                    for r in range(3):
                        g = _m_group(form, o, l, kind, 5 + (io + il + r) % 3, "normal", len(out), lw=lw, fw=fw)
                        if g is not None:
                            out.append(g)
                            break
    return out


# ---------------------------------------------------------------- family N
N_PEERS = (3, 5, 8)
N_ROLES = ("cend1", "mis1", "cmp0", "app2", "full", "hb", "stale", "below", "beyond", "snap")
N_LAST = 700   # the leader's last Index, entries past the origin


def _n_fol(role, origin, off, ldummy, llast, L, T, fwrap):
    """Followers of the N groups, by role. Merging: cmp0 starts at plo, all
    of its entries match, its log ends in chunk 0; mis1 starts in chunk 1 and
    mismatches on that chunk's last entry; app2 starts in chunk 2 with nothing
    to compare; cend1 starts in chunk 0 and its compared range ends in chunk
    1; full starts in chunk 0 and cannot hold the leader's last."""
    def tf(i):
        return TB + (i - ldummy)
    plo = origin + off
    if role == "cmp0":
        return _f(plo - 1, origin + 199, ldummy, ("merge", origin + 200, llast, None), wrap=fwrap)
    if role == "mis1":
        m = origin + 2 * CHUNK - 1
        return _f(origin + 299, m + 3, ldummy + 1, ("merge", m, llast, None), wrap=fwrap,
                  over={i: tf(i) + 20000 for i in range(m, m + 4)})
    if role == "app2":
        p = origin + 2 * CHUNK + 7
        return _f(p, p, ldummy, ("merge", p + 1, llast, None), wrap=fwrap)
    if role == "cend1":
        return _f(plo + 1, origin + 400, ldummy, ("merge", origin + 401, llast, None), wrap=fwrap)
    if role == "full":
        return _f(plo, plo + 5, llast - L, ("full", None, plo + 5, None), wrap=fwrap)
    if role == "hb":
        return _f(llast, llast, ldummy, ("hb", None, llast, None), wrap=fwrap)
    if role == "stale":
        return _f(plo + 3, plo + 3, ldummy, ("stale", None, plo + 3, None), wrap=fwrap, term=T + 1)
    if role == "below":   # compacted past prev
        return _f(plo + 2, plo + 9, plo + 6, ("below", None, plo + 9, plo + 7), wrap=fwrap)
    if role == "beyond":
        return _f(plo + 20, plo + 4, ldummy, ("beyond", None, plo + 4, plo + 5), wrap=fwrap)
    assert role == "snap"  # prev below the leader's dummy: InstallSnapshot (its own reply path)
    return _f(ldummy - 2, ldummy - 1, ldummy - 4, ("snap", None, None, None), wrap=fwrap)


def _groups_n(P):
    """P - 1 followers per group drawn from N_ROLES (every window of the
    list), the leader at peer 0, P // 2 and
    P - 1, plo at three line offsets; for P = 5 the same groups once more with
    one follower's ring misaligned by one word (the whole group in dword form)."""
    L, nf, out = 1024, P - 1, []
    merging = ("cmp0", "mis1", "app2", "cend1", "full")
    for dword in ((False, True) if P == 5 else (False,)):
        for s in range(len(N_ROLES)):
            roles = [N_ROLES[(s + i) % len(N_ROLES)] for i in range(nf)]
            if not {"cmp0", "cend1", "full"} & set(roles):
                roles[-1] = "cmp0"      # plo is set by a follower that starts in chunk 0
            for lp in (0, P // 2, P - 1):
                for off in (0, 3, 28):
                    ldummy = 600 + s
                    origin = ldummy + 10
                    llast = origin + N_LAST
                    T = TB + (llast - ldummy)
                    lwrap = origin - LINE
                    fols = []
                    for i, role in enumerate(roles):
                        mis = 1 if dword and role in merging and role == next(r for r in roles if r in merging) else 0
                        fols.append(_n_fol(role, origin, off, ldummy, llast, L, T, lwrap + 4 * i + mis))
                    out.append(_group(P, L, lp, ldummy, llast, lwrap, fols,
                                      ("dword " if dword else "") + "+".join(roles), c0=ldummy + 2,
                                      rejected="full" in roles))
    return out


# ---------------------------------------------------------------- family S
def _s_group(form, q, off, hit, kind, start_gap=0, cmp_len=None, fol_kind="merge", full_len=None, P=3):
    """A Figure-8 group: currentTerm T is above every term of the log except
    at Index `hit` (None: nowhere); the term at the leader's last is not T and
    the leader's terms descend (terms_sorted 0), so a1 scans [c0 + 1, last - 1]
    for T. `hit` counts from the chunk origin ("slo" / "shi": the window's
    ends). start_gap: how far the window starts below every follower's
    prev + 1; cmp_len: entries the merging followers already hold past prev;
    fol_kind "hb": no merging follower; full_len: one follower is
    capacity-full and the window is full_len long (the scan runs after the
    pass, wave_scan_down_eq)."""
    L, mis = form_L(form), form_mis(form)
    vec = form == "vec"
    ldummy = 1100 + q % 5
    if full_len is None:
        c0 = ldummy + 2 + q % 3
        slo = c0 + 1
        start = slo + start_gap
        plo = slo
        origin = plo - off if vec else plo
        llast = origin + 600 + q % 4
    else:
        start = ldummy + 4
        plo = start
        origin = plo - off if vec else plo
        llast = max(start + 3, ldummy + full_len + 3 + q % 2)
        c0 = llast - 1 - full_len
        slo = c0 + 1
    shi = llast - 1
    h = None if hit is None else slo if hit == "slo" else shi if hit == "shi" else \
        slo + hit[1] if isinstance(hit, tuple) else origin + hit
    if h is not None and not slo <= h <= shi:
        return None
    if llast - ldummy > L - 1:
        return None
    T = TB + 3000
    gover = {ldummy + 1: TB + 9}            # a descent below the window: the leader's terms are never sorted
    if h is not None:
        gover[h] = T
    lwrap = plo - off - LINE
    fols = []
    for i in range(P - 1):
        fwrap = lwrap + 4 * i - (mis if i == 0 else 0)
        if full_len is not None and i == 0:
            fols.append(_f(start - 1, start + 1, llast - L, ("full", None, start + 1, None), wrap=fwrap))
        elif fol_kind == "hb":
            fols.append(_f(llast, llast, ldummy, ("hb", None, llast, None), wrap=fwrap))
        else:
            keep = 0 if cmp_len is None else cmp_len
            fl = start - 1 + keep if keep >= 0 else llast + keep   # (negative: counted from the leader's last)
            fols.append(_f(start - 1, fl, ldummy, ("merge", fl + 1, llast, None), wrap=fwrap))
    return _group(P, L, q % P, ldummy, llast, lwrap, fols, kind, T=T, c0=c0, gover=gover, rejected=full_len is not None)


def _groups_s(form):
    out = []

    def add(*a, **k):
        g = _s_group(form, len(out), *a, **k)
        if g is not None:
            out.append(g)

    for io, off in enumerate(OFFS):
        for rel in RELS:                                 # the hit at each rel of the M list
            add(off, off if rel == "first" else rel, f"hit {rel}")
            add(off, off if rel == "first" else rel, f"hit {rel} cmp", cmp_len=300)
        add(off, None, "nohit")
        add(off, 400 + io, "copyonly", cmp_len=10)       # after every follower has finished comparing
        for gap in (1, 5, 40):                           # the window starts below every follower's prev + 1
            add(off, 2, "early", start_gap=gap)
            add(off, 300, "early", start_gap=gap, cmp_len=20)
            add(off, None, "early nohit", start_gap=gap)
        for hit in (3, 255, 256, 511, None, "slo", "shi"):
            add(off, hit, "nomerge", fol_kind="hb")      # no merging follower: phi = shi
        add(off, "slo", "at slo")
        add(off, "shi", "at shi")
        add(off, "shi", "at shi cmp", cmp_len=-3)
    for n in S_FULL_LENS:                                # a maybe_full group: the scan runs after the pass
        for hit in ("slo", "shi", None) + ((("slo+", n // 2),) if n > 2 else ()):
            for off in (0, 3):
                add(off, hit, f"full len{n} hit {hit}", full_len=n)
    for off in OFFS:                                     # sorted leader, term at top below T: settled
        for q in range(2):
            L = form_L(form)
            ldummy = 33 + q
            start = ldummy + 3
            llast = start + 300 + off
            lwrap = start - off - LINE if form == "vec" else start - LINE
            fols = [_f(start - 1, start - 1 + 4 * i, ldummy, ("merge", start + 4 * i, llast, None),
                       wrap=lwrap + 4 * i - (form_mis(form) if i == 0 else 0)) for i in range(2)]
            out.append(_group(3, L, (off + q) % 3, ldummy, llast, lwrap, fols, "settled", T=TB + 3000, c0=ldummy + 1))
    return out


# ---------------------------------------------------------------- family C
def _c_fol(fdummy, run, breaker, wrap_in, q):
    """A follower whose term at prev (A) differs from the leader's, with
    `run` more entries of term A directly below prev and the first other term
    at Index dummy + breaker (2 or 3), or none down to dummy + 2 ("absent":
    ConflictIndex = dummy + 1)."""
    A, Bt = 9, 8
    lo = fdummy + 2
    if breaker == "absent":
        prev = lo + run
        ci = fdummy + 1
    else:
        prev = fdummy + breaker + run + 1
        ci = fdummy + breaker
    flast = prev + q % 3
    over = {i: A for i in range(lo, flast + 1)}
    over[fdummy + 1] = Bt - 1
    if breaker != "absent":
        over[fdummy + breaker] = Bt
    wrap = prev - run // 2 if wrap_in else None         # the ring wraps inside the run (at prev for run 0)
    return _f(prev, flast, fdummy, ("scan", None, flast, ci), wrap=wrap, over=over, commit=fdummy)


def _groups_c():
    L, out = 1024, []
    for run in C_RUNS:
        for br in C_BREAKERS:
            for wrap_in in (False, True):
                q = len(out)
                D = 20 + q % 9
                f = _c_fol(D, run, br, wrap_in, q)
                out.append(_group(2, L, q % 2, D, f["prev"] + 5, D, [f], f"run{run} br{br}" + (" wrap" if wrap_in else ""),
                                  c0=D))
    for k in (2, 3, 4):                                  # several scanning followers: the probes share a round trip
        for s in range(len(C_RUNS)):
            q = len(out)
            D = 25 + q % 4
            fols = [_c_fol(D, C_RUNS[(s + 4 * i) % len(C_RUNS)], C_BREAKERS[(s + i) % 3], (s + i) % 2 == 1, q + i)
                    for i in range(k)]
            llast = max(f["prev"] for f in fols) + 3
            fols += [_f(llast, llast, D, ("hb", None, llast, None)) for _ in range(4 - k)]
            out.append(_group(5, L, q % 5, D, llast, D, fols, f"scan x{k}", c0=D))
    return out


# ---------------------------------------------------------------- family D
D_FORMS = ("vec", "mis1", "odd")
D_POS = ("first", "second", "lane64", "lane128", "chunk", "last", "absent", "outside")
D_KEEP = (0, 100, 280)   # entries the follower holds past prev: none; its compare ends in chunk 0 (the copy loop
#                          takes over at the first chunk end); its compare runs into chunk 1 (the carry stays inside
#                          the compare loop)


def _d_group(form, pos, keep, atprev, off, q):
    """One descent term(x - 1) > term(x) in the leader's log: x the first
    shipped entry (its predecessor is prevLogTerm's entry, outside the
    message), the second, a lane edge (64 and 128 entries past the origin), the
    first chunk end, the last entry, nowhere, or below prev (outside the
    message). atprev: the follower's dummy is prev (an append from the dummy's
    successor replaces its whole log)."""
    L, mis = form_L(form), form_mis(form)
    ldummy = 1100 + q % 5
    prev = ldummy + 6
    plo = prev + 1
    origin = plo - off if form == "vec" else plo
    llast = origin + 300 + q % 3
    x = {"first": plo, "second": plo + 1, "lane64": origin + WAVE, "lane128": origin + 2 * WAVE, "chunk": origin + CHUNK,
         "last": llast, "absent": None, "outside": prev - 3}[pos]
    gover = {} if x is None else {i: TB + (i - ldummy) - 2000 for i in range(x, llast + 1)}
    fdummy = prev if atprev else prev - 1 if pos == "outside" else ldummy
    flast = prev + keep
    lwrap = plo - off - LINE
    fol = _f(prev, flast, fdummy, ("merge", flast + 1, llast, None), wrap=lwrap - mis)
    return _group(2, L, q % 2, ldummy, llast, lwrap, [fol], f"desc {pos} keep{keep}" + (" atprev" if atprev else ""),
                  T=TB + 3000, c0=prev, gover=gover)   # (c0 = prev: the tick's scan window starts at plo too)


def _groups_d(form):
    out = []
    for pos in D_POS:
        for keep in D_KEEP:
            for atprev in (False, True):
                for off in (0, 3):
                    out.append(_d_group(form, pos, keep, atprev, off, len(out)))
    return out


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=8)
def case(family: str, form: str = "vec", P: int = 0) -> Case:
    """The family's groups in one form (N: one case per P, dwordx4 form with a
    dword subset at P = 5; C: dwordx4 form only, its scans never enter the
    pass). Treat the states as read-only."""
    if family == "N":
        return _assemble(f"N-P{P}", "N", "vec", P, 1024, _groups_n(P))
    if family == "C":
        gs = _groups_c()
        two = [g for g in gs if len(g["reps"]) == 2]
        return _assemble(f"C-P{P}", "C", "vec", P, 1024, two if P == 2 else [g for g in gs if len(g["reps"]) == 5])
    fn = {"M": _groups_m, "W": _groups_w, "F": _groups_f, "S": _groups_s, "D": _groups_d, "V": _groups_v}[family]
    P = 3 if family == "S" else 2
    return _assemble(f"{family}-{form}", family, form, P, form_L(form), fn(form))


# ------------------------------------------------------ the grid, restated
def _term_at(st, log, s, i, L):
    return int(log[s, (int(st["log_head"][s]) + i - int(st["dummy_index"][s])) % L])


def geometry(st: dict, lp: np.ndarray, P: int, L: int, log_off: int = 0) -> list:
    """Where the pass's decisions fall, from the state arrays, the leader
    peers and the chunk parameters alone. Per group a dict (None: no leader):
      vec       the dwordx4 form is chosen: L % 4 == 0, the log 16-B aligned (log_off % 4 == 0: words past a
                16-B boundary) and every merging follower's head - dummy equal to the leader's mod 4
      plo, origin, line   the pass's first Index, the chunk origin (dwordx4: plo minus its position in its
                128-B line of the leader's row, (ld * L + ring(plo + head - dummy)) mod 32; dword: plo),
                that position
      fols      {peer: {cls, start, cend, nend, m, full, lwrap, fwrap}}: m the first Index in [start, cend)
                whose terms differ, else cend when cend < nend ("beyond the end"), else None; lwrap / fwrap:
                the first Index in (plo, nend) at ring slot 0 of the leader's / the follower's row, or None
      settled   a1 decided by the top term alone on a sorted leader (term at top below currentTerm)
      scan      (slo, shi, hit) when a1 scans for currentTerm on the pass or after it (`late`), else None
      cscan     {peer: (run, breaker, wrap)} for ConflictIndex scans
      desc      the Indexes i in (leader dummy + 1, last] with term(i - 1) > term(i)
    and `pos(x)`: (rel, chunk, lane, u) of Index x on the grid."""
    G = len(lp)
    log = st["log_term"].reshape(G * P, L).astype(np.int64)
    out = []
    for g in range(G):
        if not 0 <= lp[g] < P:
            out.append(None)
            continue
        ld = g * P + int(lp[g])
        T, c0 = int(st["current_term"][ld]), int(st["commit_index"][ld])
        last, ldummy, lhead = int(st["last_index"][ld]), int(st["dummy_index"][ld]), int(st["log_head"][ld])
        if st["state"][ld] != LEADER or c0 < ldummy:
            out.append(None)
            continue
        nend = last + 1
        fols, cscan, words = {}, {}, []
        lt = [_term_at(st, log, ld, i, L) for i in range(ldummy, nend)]
        desc = [ldummy + k for k in range(2, len(lt)) if lt[k - 1] > lt[k]]
        vec = L % 4 == 0 and log_off % 4 == 0
        maybe_full = False
        for j in range(P):
            if j == lp[g]:
                continue
            f = g * P + j
            prev = int(st["next_index"][ld * P + j]) - 1
            ft, fdummy = int(st["current_term"][f]), int(st["dummy_index"][f])
            flast, fhead = int(st["last_index"][f]), int(st["log_head"][f])
            old = int(st["match_index"][ld * P + j])
            d = dict(start=prev + 1, cend=min(last, flast) + 1, nend=nend, m=None, full=False, lwrap=None, fwrap=None)
            if prev < ldummy:
                d["cls"] = "snap"
            elif prev > last:
                d["cls"] = "panic"
            elif T < ft:
                d["cls"] = "stale"
            elif prev < fdummy:
                d["cls"] = "below"
            elif prev > flast:
                d["cls"] = "beyond"
            elif _term_at(st, log, f, prev, L) != _term_at(st, log, ld, prev, L):
                d["cls"] = "scan" if prev > fdummy + 1 else "mismatch"
                if d["cls"] == "scan":
                    a = _term_at(st, log, f, prev, L)
                    run, i = 0, prev - 1
                    while i >= fdummy + 2 and _term_at(st, log, f, i, L) == a:
                        run, i = run + 1, i - 1
                    wrapi = fdummy + (-fhead) % L          # the first Index at or above the dummy at ring slot 0
                    cscan[j] = (run, "absent" if i < fdummy + 2 else i - fdummy,
                                wrapi > fdummy and prev - run <= wrapi <= prev)
            elif last - prev > 0:
                d["cls"] = "merge"
                vec = vec and ((fhead - fdummy) - (lhead - ldummy)) % 4 == 0
                d["full"] = last - fdummy > L - 1
                maybe_full |= d["full"]
                for i in range(d["start"], d["cend"]):
                    if _term_at(st, log, f, i, L) != _term_at(st, log, ld, i, L):
                        d["m"] = i
                        break
                else:
                    d["m"] = d["cend"] if d["cend"] < nend else None
            else:
                d["cls"] = "hb"
            if d["cls"] in ("merge", "hb"):
                words.append(max(old, last) if not d["full"] else old)
            elif d["cls"] != "snap":
                words.append(old)
            d.update(fdummy=fdummy, fhead=fhead, flast=flast)
            fols[j] = d
        if any(d["cls"] == "panic" for d in fols.values()):
            out.append(None)
            continue
        merging = [d for d in fols.values() if d["cls"] == "merge"]
        # a1 (raft_append_entry.go:88-101): top = the (P/2)-th largest matchIndex word, capped by last
        scan, settled = None, False
        nsucc = sum(d["cls"] in ("merge", "hb") and not d["full"] for d in fols.values())
        stale = any(d["cls"] == "stale" for d in fols.values())
        if nsucc and not stale and len(words) >= P // 2:
            top = min(sorted(words, reverse=True)[P // 2 - 1], last)
            if top > c0:
                t = _term_at(st, log, ld, top, L)
                settled = bool(t != T and st["terms_sorted"][ld] and t < T)
                if t != T and not settled:
                    hit = next((i for i in range(top - 1, c0, -1) if _term_at(st, log, ld, i, L) == T), None)
                    scan = dict(slo=c0 + 1, shi=top - 1, hit=hit, late=maybe_full)
        on_pass = scan is not None and not scan["late"] and scan["slo"] <= scan["shi"]
        if not merging and not on_pass:
            out.append(dict(vec=vec, plo=None, origin=None, line=None, fols=fols, scan=scan, cscan=cscan, pos=None,
                            nend=nend, settled=settled, desc=desc))
            continue
        plo = min([d["start"] for d in merging] + ([scan["slo"]] if on_pass else []))
        line = (ld * L + (plo + lhead - ldummy) % L) % LINE
        origin = plo - line if vec else plo
        phi = last if merging else scan["shi"]
        for d in fols.values():
            for key, dm, hd in (("lwrap", ldummy, lhead), ("fwrap", d["fdummy"], d["fhead"])):
                w = plo + 1 + (-(plo + 1 + hd - dm)) % L     # the first Index above plo at slot 0
                d[key] = w if w < nend else None

        def pos(x, origin=origin, vec=vec):
            rel = x - origin
            r = rel % CHUNK
            return (rel, rel // CHUNK, r // 4, rel % 4) if vec else (rel, rel // CHUNK, r % WAVE, r // WAVE)

        out.append(dict(vec=vec, plo=plo, origin=origin, line=line, phi=phi, fols=fols, scan=scan, cscan=cscan, pos=pos,
                        nend=nend, settled=settled, desc=desc))
    return out


def nend_tags(geo: dict, m: int) -> set:
    """Which of NENDS the leader's last + 1 is, relative to m and the grid."""
    nend, origin = geo["nend"], geo["origin"]
    E = origin + CHUNK * ((m - origin) // CHUNK + 1)
    cand = {"m+1": m + 1, "m+2": m + 2, "m+5": m + 5, "E": E, "E+1": E + 1, "E+256": E + CHUNK,
            "E+257": E + CHUNK + 1, "E+259": E + CHUNK + 3}
    return {k for k, v in cand.items() if v == nend}


# ------------------------------------------------- family V: buffer layouts
V_LAYOUTS = ("residue", "lastword", "shared", "word0-1", "word0-2", "word0-3")


def follower_phase(args, st, L):
    """Where, mod 4 words, the first entry of every message lands in the
    receiving follower's row (a 16-B aligned log): (slot * L + ring(head +
    prev + 1 - dummy)) mod 4."""
    f = args["slot"].astype(np.int64)
    pos = (st["log_head"][f].astype(np.int64) + args["prev_log_index"] + 1 - st["dummy_index"][f]) % L
    return ((f * L + pos) % 4).astype(np.int64)


def value_layout(args, ok, st, L, layout, eligible=None):
    """The gathered items' entries copied into one flat buffer, as the network
    would deliver them, at a chosen layout. Returns (args with entries_offset
    rebased, buffer, base_off): base_off is how many words past a 16-B
    boundary the buffer itself must be bound for the layout to mean what it
    says (0: any 16-B aligned buffer, the host path's).
      residue   item j starts j % 4 words past a 16-B boundary
      lastword  every item 16-B aligned like its follower's row (the dwordx4 form's condition); the last one
                ends on the buffer's last word, short of a 16-B boundary: its rounded-up dwordx4 would run past
      shared    the messages of one leader share one copy of its entries [min prev + 1, last]
      word0-r   as lastword's alignment, but one message whose follower phase is r begins at word 0 of a
                buffer bound r words past a 16-B boundary: its rounded-down dwordx4 would start before it
    eligible: which items may be the one lastword / word0 single out (default: any)."""
    el = np.ones(len(args), bool) if eligible is None else eligible
    a2 = args.copy()
    n = np.where(ok, args["n_entries"], 0).astype(np.int64)
    ph = follower_phase(args, st, L)
    src = st["log_term"][entry_positions(st["log_head"], L, args["entries_offset"], n)]
    first = np.cumsum(n) - n                           # item j's entries are src[first[j] : first[j] + n[j]]
    start = np.zeros(len(args), np.int64)
    base_off, cur = 0, 0
    order = list(range(len(args)))
    if layout.startswith("word0"):
        base_off = int(layout[-1])
        i0 = next(j for j in order if el[j] and n[j] > 4 and ph[j] == base_off)
        order.remove(i0)
        order.insert(0, i0)
    elif layout == "lastword":
        i0 = next(j for j in reversed(order) if el[j] and n[j] > 4 and (ph[j] + n[j]) % 4 != 0)
        order.remove(i0)
        order.append(i0)
    if layout == "shared":
        slot_of = {}
        for j in order:
            if n[j] == 0:
                continue
            key = int(args["entries_offset"][j]) // L
            slot_of.setdefault(key, []).append(j)
        buf = []
        for key, items in slot_of.items():
            jm = max(items, key=lambda j: n[j])        # the longest message: min prev
            cur = (cur + 3) // 4 * 4 + key % 4
            for j in items:
                assert args["prev_log_index"][j] + n[j] == args["prev_log_index"][jm] + n[jm]
                start[j] = cur + (n[jm] - n[j])
            buf.append((cur, src[first[jm]:first[jm] + n[jm]]))
            cur += int(n[jm]) + 5
        total = cur
    else:
        buf = []
        for k, j in enumerate(order):
            if layout == "residue":
                cur = (cur + 3) // 4 * 4 + j % 4
            elif not (k == 0 and layout.startswith("word0")):
                cur += (ph[j] - base_off - cur) % 4    # (base_off + start) % 4 == the follower's phase
            start[j] = cur
            buf.append((cur, src[first[j]:first[j] + n[j]]))
            cur += int(n[j]) + (0 if layout == "lastword" and k == len(order) - 1 else 5)
        total = cur
    out = np.full(total, POISON, np.int32)
    for at, words in buf:
        out[at:at + len(words)] = words
    a2["entries_offset"] = np.where(ok & (n > 0), start, 0)
    return a2, out, base_off


def value_geometry(args, ok, st, L, n_buf, base_off=0):
    """Per item with entries, from the message, the follower's ring words and
    the buffer's size and binding alone: `aligned` (the entries and the
    follower's row 16-B aligned alike), `head_ok` / `tail_ok` (the dwordx4
    groups holding the first / last entry lie inside the buffer), `residue`
    (entries_offset mod 4) and `vec` = L % 4 == 0 and all three (handle_one's
    choice). None for items without entries."""
    ph = follower_phase(args, st, L)
    out = []
    for j in range(len(args)):
        nj, eo = int(args["n_entries"][j]), int(args["entries_offset"][j])
        if not ok[j] or nj <= 0:
            out.append(None)
            continue
        a, z = base_off + eo, base_off + eo + nj - 1
        d = dict(residue=eo % 4, aligned=a % 4 == ph[j], head_ok=a - a % 4 >= base_off,
                 tail_ok=(z | 3) < base_off + n_buf)
        d["vec"] = L % 4 == 0 and d["aligned"] and d["head_ok"] and d["tail_ok"]
        out.append(d)
    return out


def merging_items(c: Case, slots, peers) -> np.ndarray:
    """Which (leader slot, peer) items are built to merge and be accepted."""
    return np.array([c.expect[int(s) // c.P][int(p)][0] == "merge" for s, p in zip(slots, peers)], bool)
