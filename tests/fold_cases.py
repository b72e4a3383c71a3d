"""Directed cases of the AppendEntries reply fold (mraft_process_append_replies:
processAppendEntriesReply + advanceCommitIndexForLeader,
src/raft/raft_append_entry.go:66-105), shared by tests/test_fold_cases.py (CPU:
the model below against the C oracle, and every claimed cell present in the
model's classification) and tests/test_fold_cases_gpu.py (the engine against
the oracle, bit for bit; a child process runs this file on the small-grid
library, multiraft_amd/libmraft_hip_grid1.so).

The fold is three launches (k_claim_zero, k_fold, k_fold_tail in
multiraft_amd/csrc/mraft_fold.hip): segments of at most GW = 8 replies fold
eight per wave on lane groups (the "group" path), longer ones one per wave in
batches of 64 replies through a device list (the "long" path); every a1
evaluation is a range (lo, hi) = (H + 1, top) of Indexes whose top word is
probed, settled by sorted terms, or scanned downward over [lo, hi - 1]: 512
terms per iteration from the pending list (group path), 256 inside the long
path.

Hand-built states: one leader replica per group (`Groups.add`), its log ring,
head, dummy, commit, match / next; reply batches placed so each decision falls
on a chosen reply, lane, entry and ring position. Every family is a function
returning (G, P, L, state, items, seg_begin, claims); `model_fold` restates the
fold in plain Python as the oracle states it and records, per reply, the path,
batch and lane, the a1 range and its class, and ring positions; `cells` turns
that record into cell names, and `claims` must be among them.

Cell names (A-E of the matrix): see `cells`. "tie" cells do not exist at P = 2
(a single voter cannot tie).

Run as a program: every family on the library MRAFT_LIB names against the
oracle, one JSON line {"cases": [[name, n_items, ok], ...]}, exit status 1 on
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

from cases_program import run_all, sorted_terms  # noqa: E402

from multiraft_amd._abi import (AE_RESULT, CANDIDATE, F_APPLIED, F_COMMITTED, F_NEED_MORE,  # noqa: E402
                                F_STEPPED_DOWN, FOLLOWER, ITEM_BAD_SLOT, ITEM_BAD_STATE, ITEM_DUP_SLOT, LEADER)
from multiraft_amd.engine import copy_state, new_state  # noqa: E402

GW = 8                      # replies a lane group folds; longer segments take the long path
TOP = 2**31 - 2             # the highest Index of the engine's domain
IMAX = 2**31 - 1
SCAN_GROUP = (0, 1, 62, 63, 64, 65, 510, 511, 512, 513, 1023, 1024, 1025)   # around wave_scan_down_eq<8>'s 512
SCAN_LONG = (0, 1, 62, 63, 64, 65, 254, 255, 256, 257, 511, 512, 513)       # around wave_scan_down_eq<4>'s 256
RING0 = ("lo", "lo1", "mid", "hi1", "probe")


# ---------------------------------------------------------------- states
class Groups:
    """One leader replica per group; the other replicas stay as Make left them."""

    def __init__(self, P: int, L: int):
        self.P, self.L, self.rows = P, L, []

    def add(self, log, T=5, me=0, role=LEADER, dummy=0, dterm=0, head=0, commit=None, match=None, nxt=None):
        """log: the terms of Index dummy + 1 .. last. match / nxt: {peer: value}
        (default: matchIndex = commit, nextIndex = matchIndex + 1). Returns the slot."""
        log = [int(t) for t in log]
        assert len(log) <= self.L - 1 and 0 <= me < self.P
        last = dummy + len(log)
        commit = dummy if commit is None else commit
        m = [commit] * self.P
        m[me] = 0
        m = [int((match or {}).get(j, v)) for j, v in enumerate(m)]
        nx = [v + 1 for v in m]
        nx[me] = last + 1
        nx = [int((nxt or {}).get(j, v)) for j, v in enumerate(nx)]
        self.rows.append(dict(log=log, T=T, me=me, role=role, dummy=dummy, dterm=dterm, head=head % self.L,
                              commit=commit, m=m, nx=nx, last=last))
        return (len(self.rows) - 1) * self.P + me

    def state(self) -> dict:
        G, P, L = len(self.rows), self.P, self.L
        st = new_state(G, P, L)
        for g, r in enumerate(self.rows):
            s = g * P + r["me"]
            st["current_term"][s], st["state"][s] = r["T"], r["role"]
            st["dummy_index"][s], st["last_index"][s] = r["dummy"], r["last"]
            st["commit_index"][s], st["last_applied"][s] = r["commit"], min(r["commit"], r["dummy"])
            st["log_head"][s] = r["head"]
            terms = np.array([r["dterm"]] + r["log"], np.int32)
            st["log_term"][s * L + (r["head"] + np.arange(len(terms))) % L] = terms
            st["match_index"][s * P:(s + 1) * P] = r["m"]
            st["next_index"][s * P:(s + 1) * P] = r["nx"]
        st["terms_sorted"] = sorted_terms(st, G, P, L)
        return st


def rec(slot, peer, T, prev, n=0, ok=1, rt=None, ci=0):
    """One reply record: args (term T, prevLogIndex prev, n entries) and the reply."""
    return (slot, peer, T, prev, n, T if rt is None else rt, ok, ci)


def batch(segs, head=0, tail=0):
    """segs: lists of records. head / tail: records no segment covers."""
    flat, sb = [rec(0, 1, 1, 0)] * head, [head]
    for s in segs:
        flat += s
        sb.append(len(flat))
    flat += [rec(0, 1, 1, 0)] * tail
    items = np.zeros(len(flat), dtype=AE_RESULT)
    for i, r in enumerate(flat):
        items[i] = r
    return items, np.array(sb, np.int64)


def stale(slot, T, k, peer=1):
    """k replies of an older term: ignored (flag 0), any lane."""
    return [rec(slot, peer, T, 0, 0, 1, rt=T - 1)] * k


def wrap(path, recs, slot, T, pre=3, peer=1):
    """The records as a group-path segment, or padded with ignored replies to
    a long one with the first record at reply `pre`."""
    if path == "group":
        assert len(recs) <= GW
        return list(recs)
    out = stale(slot, T, pre, peer) + list(recs)
    return out + stale(slot, T, max(0, GW + 1 - len(out)), peer)


def live_seg(gs: Groups, n: int, T=5, head=0, me=0):
    """A group and a segment of n replies for it, every one with a non-zero
    flag: n - 1 heartbeat successes (APPLIED) and a success that commits the
    last entry (APPLIED | COMMITTED), so a skipped or twice-folded segment shows."""
    P = gs.P
    slot = gs.add([T - 1, T - 1, T], T=T, head=head, me=me, commit=1, dummy=0)
    peers = [j for j in range(P) if j != me]
    out = [rec(slot, peers[k % len(peers)], T, 1, 0) for k in range(n - 1)]
    # P // 2 peers acknowledge Index 3; the last of them commits it
    need = peers[:P // 2]
    out = out[:max(0, n - len(need))] + [rec(slot, p, T, 1, 2) for p in need][-n:]
    return slot, out


# ---------------------------------------------------------------- the model
def model_fold(G, P, L, st, items, seg_begin):
    """The fold as the oracle states it (:66-105 on the replicas in segment
    order, rejections first), on a copy of `st`. Returns (flags, err, state,
    trace); trace = {"segs": [...], "replies": [...], "pending": n, "long": n}."""
    st = copy_state(st)
    n = len(items)
    ns = n if seg_begin is None else len(seg_begin) - 1
    gp = G * P
    flags, err = np.zeros(n, np.int32), np.zeros(n, np.int32)
    bounds = [(i, i + 1) if seg_begin is None else (int(seg_begin[i]), int(seg_begin[i + 1])) for i in range(ns)]
    owner = {}
    for sg, (b, e) in enumerate(bounds):
        if b < e:
            s0 = int(items["slot"][b])
            if 0 <= s0 < gp:
                owner.setdefault(s0, sg)
    segs, reps = [], []
    covered = np.zeros(n, bool)
    pending = longs = 0
    npush = 0
    for sg, (b, e) in enumerate(bounds):
        cnt = max(0, e - b)
        path = "empty" if cnt == 0 else "group" if cnt <= GW else "long"
        S = dict(sg=sg, b=b, n=cnt, path=path, wave=sg // GW, gpos=sg % GW, err=0, why=None, at=None, slot=None,
                 stepdown_in=False, applied=0, nranges=0, owner=None)
        segs.append(S)
        if cnt == 0:
            continue
        covered[b:e] = True
        longs += path == "long"
        it = items[b:e]
        slot = int(it["slot"][0])
        S["slot"] = slot
        bad = 0
        if not 0 <= slot < gp:
            bad, S["why"] = ITEM_BAD_SLOT, "first_slot_oob"
        elif owner[slot] != sg:
            bad, S["why"], S["owner"] = ITEM_DUP_SLOT, "dup", owner[slot]
        else:
            me = slot % P
            for k in range(cnt):
                r = it[k]
                why = ("other_slot" if int(r["slot"]) != slot else "peer_neg" if r["peer"] < 0 else
                       "peer_ge_P" if r["peer"] >= P else "peer_me" if r["peer"] == me else
                       "n_neg" if r["args_n_entries"] < 0 else
                       "idx_top" if int(r["args_prev_log_index"]) + int(r["args_n_entries"]) > TOP else None)
                if why:
                    bad = ITEM_BAD_SLOT
                    if S["why"] is None:
                        S["why"], S["at"] = why, k
            if not bad and st["commit_index"][slot] < st["dummy_index"][slot]:
                bad, S["why"] = ITEM_BAD_STATE, "bad_state"
        if bad:
            S["err"] = bad
            err[b:e] = bad
            if 0 <= slot < gp:
                S["stepdown_in"] = bool((it["reply_term"].astype(np.int64) > int(st["current_term"][slot])).any())
            continue
        me = slot % P
        last, dummy, head = int(st["last_index"][slot]), int(st["dummy_index"][slot]), int(st["log_head"][slot])
        srt = int(st["terms_sorted"][slot])
        row = st["log_term"][slot * L:(slot + 1) * L]
        rp = lambda i: (head + i - dummy) % L  # noqa: E731
        t0, H = int(st["current_term"][slot]), int(st["commit_index"][slot])
        S["role0"], S["c0"] = int(st["state"][slot]), H
        m, nx = st["match_index"][slot * P:(slot + 1) * P], st["next_index"][slot * P:(slot + 1) * P]
        m0, nx0 = m.copy(), nx.copy()
        seen = {}
        stepped = None
        for k in range(cnt):
            r = it[k]
            p, at, ap, an = int(r["peer"]), int(r["args_term"]), int(r["args_prev_log_index"]), int(r["args_n_entries"])
            rt, ok, ci = int(r["reply_term"]), int(r["reply_success"]), int(r["reply_conflict_index"])
            term, role = int(st["current_term"][slot]), int(st["state"][slot])
            R = dict(i=b + k, sg=sg, k=k, path=path, batch=k // 64 if path == "long" else 0,
                     lane=k % 64, slot=slot, P=P, fl=0, kind=None, cls="none", rng=None, d=None, srt=srt,
                     after_stepdown=stepped is not None, top_term=None, looks_ok=False, t0=t0,
                     idx_top_ok=ap + an == TOP)
            R["looks_ok"] = bool(ok and at == t0 and ap == int(nx[p]) - 1 and rt == t0)
            fl = 0
            if rt > term:                                                   # :67-72
                st["current_term"][slot], st["voted_for"][slot], st["state"][slot] = rt, -1, FOLLOWER
                st["persist_dirty"][slot] |= 1
                fl = F_STEPPED_DOWN
                R["kind"] = "stepdown"
                stepped = k if stepped is None else stepped
            elif rt == term and role == LEADER and at == term and ap == int(nx[p]) - 1:   # :73-74
                fl = F_APPLIED
                S["applied"] += 1
                if p in seen:
                    R["repeat"] = "prev_updated" if seen[p] else "prev_same"
                if ok:
                    R["kind"] = "success"
                    old = int(m[p])
                    m[p] = an + ap                                          # :76
                    nx[p] = an + ap + 1                                     # :77
                    R["match_down"] = an + ap < old
                    # a1 as Go states it (:89-105)
                    hit = None
                    others = [int(m[j]) for j in range(P) if j != me]
                    for i in range(last, int(st["commit_index"][slot]), -1):
                        if sum(v >= i for v in others) + 1 > P // 2 and int(row[rp(i)]) == term:
                            hit = i
                            break
                    if hit is not None:
                        st["commit_index"][slot] = hit                      # :99
                        fl |= F_COMMITTED
                    # ... and as the kernels partition it: the range (H, top]
                    q = sorted(others, reverse=True)[P // 2 - 1]
                    top = min(q, last)
                    R.update(q=q, top=top, last=last, others=others, self_m=int(m[me]), H=H)
                    x = None
                    if top > H:
                        lo, hi = H + 1, top
                        pv = int(row[rp(hi)])
                        R["rng"], R["top_term"] = (lo, hi), pv
                        R["ring"] = dict(lo=rp(lo), hi1=rp(hi - 1), probe=rp(hi), lo1=rp(lo + 1), mid=rp((lo + hi) // 2))
                        R["c_term"] = int(row[rp(lo - 1)]) if lo - 1 >= dummy else None
                        R["below_c_term"] = any(int(row[rp(i)]) == t0 for i in range(max(dummy, lo - 4), lo - 1))
                        R["commit_eq_dummy"] = lo - 1 == dummy and dummy > 0
                        S["nranges"] += 1
                        if pv == t0:
                            x, R["cls"] = hi, "probe"
                        elif srt and pv < t0:
                            R["cls"] = "settled"
                        elif lo == hi:
                            R["cls"] = "len1miss"
                        else:
                            R["cls"] = "scanmiss"
                            for i in range(hi - 1, lo - 1, -1):
                                if int(row[rp(i)]) == t0:
                                    x, R["cls"], R["d"] = i, "scanhit", hi - 1 - i
                                    break
                            if path == "group":
                                R["pend_pos"] = npush
                                npush += 1
                                pending += 1
                        H = top
                    # the closed form: the range's result is Go's
                    assert x == hit, ("the range argument fails", sg, k, x, hit)
                else:
                    R["kind"] = "fail"
                    nx[p] = ci                                              # :82
                seen[p] = seen.get(p, False) or int(nx[p]) != int(nx0[p])
                R["nm"] = int(nx[p]) - (last + 1)
                if int(nx[p]) < last + 1:                                   # :84-86
                    fl |= F_NEED_MORE
            else:
                R["kind"] = ("stale_reply" if rt < term else "not_leader" if role != LEADER else
                             "args_term" if at != term else "prev_mismatch")
                if R["kind"] == "prev_mismatch" and p in seen and seen[p] and ap == int(nx0[p]) - 1:
                    R["repeat"] = "stale_prev"
            R["fl"] = fl
            flags[b + k] = fl
            reps.append(R)
        S["stepped"] = stepped
        S["unchanged_mn"] = bool((m == m0).all() and (nx == nx0).all())
    tr = dict(segs=segs, replies=reps, pending=pending, long=longs, n=n, ns=ns, P=P, G=G, L=L,
              null_sb=seg_begin is None, flags=flags, err=err,
              uncovered_head=bool(n and not covered[0]), uncovered_tail=bool(n and not covered[-1]))
    return flags, err, st, tr


def cells(tr) -> set:
    """The matrix cells a call contains, from the model's record.

    A: A.len<n>.<path>, A.empty_between, A.null_seg_begin, A.uncovered_head/_tail, A.nseg<n>, A.waves<w>,
       A.long_at<pos> (one long segment at that group position of a wave, short ones around it),
       A.wave_long<c> (c segments of one wave long), A.long_gt16, A.pending_gt1024, A.all_live
    B: B.<reason>.<path>[.k0|.klast|.k63|.k64] with a normally folding neighbour in the wave,
       B.idx_top_ok.<path>, B.dup.same_wave / other_wave / of_rejected / group_beats_long / long_beats_group,
       B.bad_state.<path>, B.rejected_stepdown.<path>, B.P1
    C: C.stepdown.<first|middle|last>.<path>, C.ignored_success_after_stepdown.<path>, C.stepdown.k63/k64.long,
       C.<stale_reply|args_term|prev_mismatch>.<path>, C.nonleader_stepdown.<role>.<path>,
       C.nonleader_ignored.<role>.<path>, C.success/.fail.<path>, C.need_more.set_at_last / clear_at_last1.<path>,
       C.repeat.prev_updated / stale_prev.<path>, C.match_down.<path>, C.nothing_applied.<path>
    D: D.P<P>.tie / self_high / self_low / clipped / no_range (.<path>)
    E: E.<path>.len1_hit / len1_miss / probe_hit / settled / sorted_top_above.scan_hit / unsorted_top_below.scan,
       E.<path>.n<len>.miss / n<len>.hit_lo / d<dist>.hit / hit_hi1, E.<path>.term_at_commit / term_below_commit,
       E.<path>.commit_eq_dummy, E.<path>.ring0.<lo|lo1|mid|hi1|probe>, E.<path>.wraps, E.<path>.ranges<2|3>,
       E.<path>.multi.<lower>_<upper>, E.group.multi.scanhit_scanhit.two_waves, E.<path>.term_max,
       E.<path>.index_top, E.iter2.<path> (a scan's second iteration), E.upper_vectors.<path> (a hit in load
       vectors u >= 2 of an iteration), E.long.batch1.scan (a scan in a long segment's second batch)"""
    out = set()
    segs, reps = tr["segs"], tr["replies"]
    P = tr["P"]
    by_seg = {}
    for R in reps:
        by_seg.setdefault(R["sg"], []).append(R)
    nonzero = lambda S: S["err"] != 0 or any(R["fl"] for R in by_seg.get(S["sg"], []))  # noqa: E731
    folds = lambda S: S["n"] and not S["err"] and any(R["fl"] for R in by_seg.get(S["sg"], []))  # noqa: E731
    # ---- A
    for S in segs:
        out.add(f"A.len{S['n']}.{S['path']}")
    for a, b_, c in zip(segs, segs[1:], segs[2:]):
        if a["n"] and not b_["n"] and c["n"]:
            out.add("A.empty_between")
    if tr["null_sb"]:
        out.add("A.null_seg_begin")
    if tr["uncovered_head"] and tr["flags"][0] == 0 and tr["err"][0] == 0:
        out.add("A.uncovered_head")
    if tr["uncovered_tail"] and tr["flags"][-1] == 0 and tr["err"][-1] == 0:
        out.add("A.uncovered_tail")
    out.add(f"A.nseg{tr['ns']}")
    out.add(f"A.waves{(tr['ns'] + GW - 1) // GW}")
    waves = {}
    for S in segs:
        waves.setdefault(S["wave"], []).append(S)
    for w, ss in waves.items():
        lg = [S for S in ss if S["path"] == "long"]
        if len(lg) == 1 and len(ss) == GW and all(S["path"] == "group" for S in ss if S is not lg[0]):
            out.add(f"A.long_at{lg[0]['gpos']}")
        if len(lg) > 1:
            out.add(f"A.wave_long{len(lg)}")
    if tr["long"] > 16:
        out.add("A.long_gt16")
    if tr["pending"] > 1024:
        out.add("A.pending_gt1024")
    if all(nonzero(S) for S in segs if S["n"]):
        out.add("A.all_live")
    # ---- B
    for S in segs:
        if not S["err"]:
            continue
        if P == 1:
            out.add("B.P1")
            continue
        if not any(folds(N) for N in waves[S["wave"]]):
            continue                 # no neighbour in the wave folds normally: the cell does not count
        why, path = S["why"], S["path"]
        if why == "dup":
            O = segs[S["owner"]]
            out.add("B.dup.same_wave" if O["wave"] == S["wave"] else "B.dup.other_wave")
            if O["err"]:
                out.add("B.dup.of_rejected")
            if O["path"] != path and not O["err"]:
                out.add(f"B.dup.{O['path']}_beats_{path}")
        elif why in ("first_slot_oob", "bad_state"):
            out.add(f"B.{why}.{path}")
        else:
            k = S["at"]
            pos = [f"k{k}"] if k in (0, 63, 64) else []
            if k == S["n"] - 1:
                pos.append("klast")
            for q in pos or ["kmid"]:
                out.add(f"B.{why}.{path}.{q}")
        if S["stepdown_in"]:
            out.add(f"B.rejected_stepdown.{path}")
    # ---- C, D, E per reply
    role_name = {FOLLOWER: "follower", CANDIDATE: "candidate"}
    for S in segs:
        rs = by_seg.get(S["sg"], [])
        if not rs:
            continue
        path = S["path"]
        if S["applied"] == 0 and S["stepped"] is None and S["unchanged_mn"]:
            out.add(f"C.nothing_applied.{path}")
        if S["stepped"] is not None:
            k = S["stepped"]
            out.add(f"C.stepdown.{'first' if k == 0 else 'last' if k == S['n'] - 1 else 'middle'}.{path}")
            if k in (63, 64) and path == "long":
                # the replies after it, across the batch edge, would have applied under the old role
                if any(R["k"] >= 64 and R["looks_ok"] and R["fl"] == 0 for R in rs):
                    out.add(f"C.stepdown.k{k}.long")
            if any(R["k"] > k and R["looks_ok"] and R["fl"] == 0 for R in rs):
                out.add(f"C.ignored_success_after_stepdown.{path}")
            if S["role0"] != LEADER:
                out.add(f"C.nonleader_stepdown.{role_name[S['role0']]}.{path}")
        if S["role0"] != LEADER and any(R["kind"] == "not_leader" and R["looks_ok"] for R in rs):
            out.add(f"C.nonleader_ignored.{role_name[S['role0']]}.{path}")
        if S["nranges"] in (2, 3):
            out.add(f"E.{path}.ranges{S['nranges']}")
        rg = [R for R in rs if R["rng"]]
        for a, b_ in zip(rg, rg[1:]):
            short = {"probe": "probehit", "scanmiss": "scanmiss", "scanhit": "scanhit"}
            if a["cls"] in short and b_["cls"] in short:
                out.add(f"E.{path}.multi.{short[a['cls']]}_{short[b_['cls']]}")
                if (a["cls"], b_["cls"]) == ("scanhit", "scanhit") and path == "group" and tr["ns"] <= GW \
                        and a["pend_pos"] // 4 != b_["pend_pos"] // 4:
                    out.add("E.group.multi.scanhit_scanhit.two_waves")
    for R in reps:
        path, kind = R["path"], R["kind"]
        if R["after_stepdown"]:
            continue
        if kind in ("stale_reply", "args_term", "prev_mismatch"):
            out.add(f"C.{kind}.{path}")
        if kind in ("success", "fail"):
            out.add(f"C.{kind}.{path}")
            if R["nm"] == -1:
                out.add(f"C.need_more.set_at_last.{path}")
            if R["nm"] == 0:
                out.add(f"C.need_more.clear_at_last1.{path}")
        if R.get("repeat") in ("prev_updated", "stale_prev"):
            out.add(f"C.repeat.{R['repeat']}.{path}")
        if R.get("idx_top_ok"):
            out.add(f"B.idx_top_ok.{path}")
        if kind != "success":
            continue
        if R["match_down"] and not R["rng"]:
            out.add(f"C.match_down.{path}")
        # D: the order statistic
        q, oth = R["q"], R["others"]
        pre = f"D.P{R['P']}."
        if oth.count(q) >= 2:
            out.add(pre + "tie")
            out.add(pre + "tie." + path)
        withme = sorted(oth + [R["self_m"]], reverse=True)[R["P"] // 2 - 1]
        if R["self_m"] > max(oth) and withme != q and min(withme, R["last"]) > R["H"]:
            out.add(pre + "self_high")      # counting the leader's own entry would move the range
        if R["self_m"] < min(oth) and R["rng"]:
            out.add(pre + "self_low")
        if q > R["last"] and R["rng"]:
            out.add(pre + "clipped")
        if R["top"] <= R["H"]:
            out.add(pre + "no_range")
            out.add(pre + "no_range." + path)
        # E
        if not R["rng"]:
            continue
        lo, hi = R["rng"]
        n, cls, E = hi - lo, R["cls"], f"E.{path}."
        U = 512 if path == "group" else 256
        if lo == hi:
            out.add(E + ("len1_hit" if cls == "probe" else "len1_miss" if cls == "len1miss" else "len1_settled"))
        elif cls == "probe":
            out.add(E + "probe_hit")
        if cls == "settled":
            out.add(E + "settled")
        if cls in ("scanhit", "scanmiss"):
            if R["srt"] and R["top_term"] > R["t0"] and cls == "scanhit":
                out.add(E + "sorted_top_above.scan_hit")
            if not R["srt"] and R["top_term"] < R["t0"]:
                out.add(E + "unsorted_top_below.scan")
            if cls == "scanmiss":
                out.add(E + f"n{n}.miss")
            else:
                out.add(E + f"d{R['d']}.hit")
                if R["d"] == n - 1:
                    out.add(E + f"n{n}.hit_lo")
                if R["d"] == 0:
                    out.add(E + "hit_hi1")
                if R["d"] >= U:
                    out.add(f"E.iter2.{path}")
                if R["d"] % U >= 128:
                    out.add(f"E.upper_vectors.{path}")
            if R["batch"] == 1:
                out.add(E + "batch1.scan")
            if cls == "scanmiss" and n > U:
                out.add(f"E.iter2.{path}")
            if R["c_term"] == R["t0"]:
                out.add(E + "term_at_commit")
            if R["below_c_term"]:
                out.add(E + "term_below_commit")
            if R["commit_eq_dummy"]:
                out.add(E + "commit_eq_dummy")
            if n >= 4:
                for name in RING0:
                    if R["ring"][name] == 0:
                        out.add(E + "ring0." + name)
            if R["ring"]["lo"] > R["ring"]["hi1"]:
                out.add(E + "wraps")
            if R["t0"] == IMAX:
                out.add(E + "term_max")
            if R["last"] == TOP:
                out.add(E + "index_top")
    return out


# ---------------------------------------------------------------- families
def fam_lengths():
    """A: segment lengths around the list threshold (8 / 9) and fold_segment's
    batches (64, 128), an empty segment between two live ones."""
    gs = Groups(3, 16)
    segs = []
    lens = (1, 0, 7, 8, 9, 63, 64, 65, 128, 129, 1)
    for j, n in enumerate(lens):
        segs.append(live_seg(gs, n, head=j)[1] if n else [])
    items, sb = batch(segs)
    claims = {f"A.len{n}.{'empty' if n == 0 else 'group' if n <= GW else 'long'}" for n in lens}
    return len(gs.rows), 3, 16, gs.state(), items, sb, claims | {"A.empty_between", "A.all_live"}


def fam_nseg(ns):
    """A: ns live segments of one or two replies: the last wave partly live,
    and the wave count's per / rem split of the XCD remap."""
    gs = Groups(3, 16)
    segs = [live_seg(gs, 1 + j % 2, head=j, me=j % 3)[1] for j in range(ns)]
    items, sb = batch(segs)
    return ns, 3, 16, gs.state(), items, sb, {f"A.nseg{ns}", f"A.waves{(ns + GW - 1) // GW}", "A.all_live"}


def fam_null():
    """A: seg_begin == NULL (one item per segment), 20 items."""
    gs = Groups(3, 16)
    segs = [live_seg(gs, 1, head=j)[1] for j in range(20)]
    items, _ = batch(segs)
    return 20, 3, 16, gs.state(), items, None, {"A.null_seg_begin", "A.all_live", "A.nseg20"}


def fam_uncovered():
    """A: items before seg_begin[0] and after seg_begin[n_seg]: flag 0, error 0."""
    gs = Groups(3, 16)
    segs = [live_seg(gs, 1 + 4 * (j % 3), head=j)[1] for j in range(10)]
    items, sb = batch(segs, head=2, tail=3)
    return 10, 3, 16, gs.state(), items, sb, {"A.uncovered_head", "A.uncovered_tail", "A.all_live"}


def fam_longpos():
    """A: a long segment at each of the eight group positions of a wave, then
    two and all eight segments of a wave long: 18 long segments in the call."""
    gs = Groups(3, 16)
    segs = []
    for w in range(8):
        for p in range(8):
            segs.append(live_seg(gs, 9 + w if p == w else 1 + (p + w) % 8, head=w + p)[1])
    for p in range(8):
        segs.append(live_seg(gs, 12 if p in (2, 5) else 3, head=p)[1])
    for p in range(8):
        segs.append(live_seg(gs, 9 + 9 * p, head=p)[1])
    items, sb = batch(segs)
    claims = {f"A.long_at{p}" for p in range(8)} | {"A.wave_long2", "A.wave_long8", "A.long_gt16", "A.all_live"}
    return len(gs.rows), 3, 16, gs.state(), items, sb, claims


def _scan_group(gs, path, n, kind, j, T=5, dist_pad=3):
    """One group whose single successful reply opens an a1 range scanned over
    n entries [lo, hi - 1]: kind "hit_lo" (currentTerm at lo only), "miss", or
    "dist" (hit n below hi - 1, in a range dist_pad longer, a second entry of
    currentTerm below the hit). An entry of currentTerm sits at commitIndex and
    one below it (ignored; it also makes the log unsorted, so nothing settles).
    Ring position 0 falls on lo, lo + 1, the middle, hi - 1 or the probe by j."""
    d = n
    if kind == "dist":
        n = d + dist_pad
    c = 3                                  # commitIndex; lo = 4
    lo, hi = c + 1, c + 1 + n              # probe at hi
    log = [T - 2, T, T]                    # Index 1..3: currentTerm below and at commitIndex
    body = [T - 1] * n                     # Index lo .. hi - 1
    if kind == "hit_lo" and n:
        body[0] = T
    if kind == "dist":
        body[n - 1 - d] = T
        if n - 1 - d > 0:
            body[0] = T
    log += body + [T - 1 if kind != "len1hit" else T, T - 1]   # the probe word, one more entry
    target = dict(lo=lo, lo1=lo + 1, mid=(lo + hi) // 2, hi1=hi - 1, probe=hi)[RING0[j % 5]]
    slot = gs.add(log, T=T, head=-target, commit=c, match={1: c, 2: c}, nxt={1: c + 1, 2: c + 1})
    r = [rec(slot, 1, T, c, hi - c)]
    # the long path: the reply at lanes 0..60 of the first batch, every fourth in the second batch
    return wrap(path, r, slot, T, pre=(j * 7) % 61 + (64 if j % 4 == 3 else 0))


def fam_scan(L):
    """E: both scans at capacity L. Group path: lengths and hit distances around
    wave_scan_down_eq<8>'s 512 terms per iteration; long path: around
    wave_scan_down_eq<4>'s 256; both 0, 1, 62..65. Per value: the range of that
    length with its only hit at lo, the miss over that length, the hit at that
    distance below hi - 1."""
    gs = Groups(3, L)
    segs, claims = [], set()
    j = 0
    for path, vals in (("group", SCAN_GROUP), ("long", SCAN_LONG)):
        E = f"E.{path}."
        for v in vals:
            if v == 0:
                segs.append(_scan_group(gs, path, 0, "len1hit", j)); j += 1
                segs.append(_scan_group(gs, path, 0, "miss", j)); j += 1
                claims |= {E + "len1_hit", E + "len1_miss"}
            else:
                segs.append(_scan_group(gs, path, v, "hit_lo", j)); j += 1
                segs.append(_scan_group(gs, path, v, "miss", j)); j += 1
                claims |= {E + f"n{v}.hit_lo", E + f"n{v}.miss"}
            segs.append(_scan_group(gs, path, v, "dist", j)); j += 1
            claims |= {E + f"d{v}.hit"}
        claims |= {E + "ring0." + r for r in RING0}
        claims |= {E + "term_at_commit", E + "term_below_commit", E + "hit_hi1", E + "unsorted_top_below.scan",
                   f"E.iter2.{path}", f"E.upper_vectors.{path}"}
    claims.add("E.long.batch1.scan")
    items, sb = batch(segs)
    return len(gs.rows), 3, L, gs.state(), items, sb, claims


def fam_pending():
    """A: 1,100 group-path segments with an open a1 range each (hit and miss
    alternating): more than 1,024 pending ranges in the call."""
    gs = Groups(3, 16)
    segs = []
    for j in range(1100):
        segs.append(_scan_group(gs, "group", 1 + j % 7, ("hit_lo", "miss", "dist")[j % 3], j))
    for s in segs:
        assert len(s) == 1
    # a miss leaves flag APPLIED: every segment still has a non-zero flag
    items, sb = batch(segs)
    return len(gs.rows), 3, 16, gs.state(), items, sb, {"A.pending_gt1024", "A.all_live", "A.waves138"}


def fam_reject():
    """B: every rejection beside a segment of the same wave that folds normally."""
    P, L, T = 3, 16, 5
    gs = Groups(P, L)
    segs, claims = [], set()
    good = lambda n=2: live_seg(gs, n, head=len(gs.rows))[1]  # noqa: E731

    def bad_record(path, why, where):
        slot, s = live_seg(gs, {"group": 5, "long": 70}[path], head=len(gs.rows))
        k = {"k0": 0, "klast": len(s) - 1, "k63": 63, "k64": 64}[where]
        r = list(s[k])
        if why == "other_slot":
            r[0] = slot + P if k else slot    # record 0 names the segment's slot: there the bad peer stands in
            if k == 0:
                r[1] = -1
                why = "peer_neg"
        elif why == "peer_neg":
            r[1] = -1
        elif why == "peer_ge_P":
            r[1] = P
        elif why == "peer_me":
            r[1] = slot % P
        elif why == "n_neg":
            r[4] = -1
        elif why == "idx_top":
            r[3], r[4] = TOP - 4, 5
        s[k] = tuple(r)
        claims.add(f"B.{why}.{path}.{where}")
        return s

    plan = []
    for path, wheres in (("group", ("k0", "klast")), ("long", ("k0", "k63", "k64", "klast"))):
        for where in wheres:
            for why in ("other_slot", "peer_neg", "peer_ge_P", "peer_me"):
                plan.append((path, why, where))
        plan += [(path, "n_neg", "klast"), (path, "idx_top", "klast"), (path, "n_neg", "k0"), (path, "idx_top", "k0")]
    for j, a in enumerate(plan):
        segs.append(good(1 + j % 8))
        segs.append(bad_record(*a))
    # the boundary Index 2^31 - 2 is accepted (prev does not match: the record is in the domain, and ignored)
    for path in ("group", "long"):
        slot, s = live_seg(gs, {"group": 3, "long": 11}[path], head=1)
        s[0] = rec(slot, 1, T, TOP - 4, 4)
        segs += [good(), s]
    # first record's slot out of range, both signs, both paths
    for path, bs in (("group", -1), ("group", None), ("long", -7), ("long", None)):
        n = 2 if path == "group" else 10
        segs += [good(), ("oob", bs, n)]          # filled in below, once the engine's size is known
        claims.add(f"B.first_slot_oob.{path}")
    # commitIndex < dummyIndex
    for path in ("group", "long"):
        slot = gs.add([T, T, T], T=T, dummy=4, commit=3, match={1: 4, 2: 4})
        segs += [good(), wrap(path, [rec(slot, 1, T, 4, 2)], slot, T)]
        claims.add(f"B.bad_state.{path}")
    # a rejected segment with a step-down reply in it: no state change
    for path in ("group", "long"):
        slot, s = live_seg(gs, {"group": 4, "long": 12}[path], head=2)
        s[1] = rec(slot, 1, T, 1, 0, rt=T + 3)
        s[-1] = rec(slot, 5, T, 1, 0)
        segs += [good(), s]
        claims.add(f"B.rejected_stepdown.{path}")
    # duplicates: in the same wave, in another wave, of a rejected segment, group before long and long before group
    while len(segs) % GW:
        segs.append(good())
    sa, a = live_seg(gs, 3, head=3)
    sb_, b_ = live_seg(gs, 12, head=4)
    sc, c = live_seg(gs, 2, head=5)
    c[1] = rec(sc, 7, T, 1, 0)                               # rejected itself, still owns its slot
    sd, d = live_seg(gs, 2, head=6)
    w0 = [a, good(), [rec(sa, 1, T, 1, 2)] * 10, b_, c, [rec(sc, 1, T, 1, 2)], [rec(sb_, 1, T, 1, 2)], d]
    segs += w0
    segs += [good(), [rec(sd, 1, T, 1, 2)], good(), [rec(sa, 2, T, 1, 2)] * 9, good(3), good(), good(), good()]
    claims |= {"B.dup.same_wave", "B.dup.other_wave", "B.dup.of_rejected", "B.dup.group_beats_long",
               "B.dup.long_beats_group", "B.idx_top_ok.group", "B.idx_top_ok.long"}
    gp = len(gs.rows) * P
    for i, s in enumerate(segs):
        if isinstance(s, tuple):
            _, bs, n = s
            segs[i] = [rec(gp if bs is None else bs, 1, T, 1, 2)] + [rec(0, 1, T, 1, 0)] * (n - 1)
    items, sb = batch(segs)
    return len(gs.rows), P, L, gs.state(), items, sb, claims


def fam_p1():
    """B: a P = 1 engine: every record is MRAFT_ITEM_BAD_SLOT."""
    gs = Groups(1, 16)
    slots = [gs.add([5, 5], T=5, commit=0) for _ in range(4)]
    segs = [[rec(slots[0], 0, 5, 0, 1)], [rec(slots[1], 1, 5, 0, 1)] * 2, [rec(slots[2], -1, 5, 0, 1)] * 9,
            [rec(slots[3], 0, 5, 0, 1)] * 3]
    items, sb = batch(segs)
    return 4, 1, 16, gs.state(), items, sb, {"B.P1"}


def fam_a2():
    """C: the decisions of processAppendEntriesReply, in both paths."""
    P, L, T = 3, 16, 5
    gs = Groups(P, L)
    segs, claims = [], set()
    log = [T - 1] * 6 + [T] * 4            # Index 1..10, last = 10
    mk = lambda **kw: gs.add(log, T=T, head=len(gs.rows) * 3, **dict(dict(commit=2, match={1: 2, 2: 2}), **kw))  # noqa: E731
    for path in ("group", "long"):
        # step-down at the first, a middle and the last reply; a success after it is ignored
        for where in ("first", "middle", "last"):
            s = mk()
            body = [rec(s, 1, T, 2, 1), rec(s, 2, T, 2, 0), rec(s, 1, T, 3, 2), rec(s, 2, T, 2, 6)]
            k = {"first": 0, "middle": 2, "last": None}[where]
            if path == "long":
                body = body[:2] + stale(s, T, 7) + body[2:]
                k = {"first": 0, "middle": 5, "last": None}[where]
            if k is None:
                body.append(rec(s, 1, T, 5, 0, rt=T + 2))
            else:
                body.insert(k, rec(s, 2, T, 2, 0, rt=T + 1))
            segs.append(body)
            claims.add(f"C.stepdown.{where}.{path}")
        claims.add(f"C.ignored_success_after_stepdown.{path}")
        # ignored replies, each in a segment that applies nothing
        for kind, r in (("stale_reply", lambda s: rec(s, 1, T, 2, 1, rt=T - 1)),
                        ("args_term", lambda s: rec(s, 1, T - 1, 2, 1, rt=T)),
                        ("prev_mismatch", lambda s: rec(s, 1, T, 3, 1))):
            s = mk()
            segs.append(wrap(path, [r(s), rec(s, 2, T, 2, 3)], s, T))      # the neighbour reply applies
            s = mk()
            segs.append(wrap(path, [r(s)], s, T))
            claims.add(f"C.{kind}.{path}")
        claims.add(f"C.nothing_applied.{path}")
        # a Follower or Candidate at the start: only the step-down applies
        for role, name in ((FOLLOWER, "follower"), (CANDIDATE, "candidate")):
            s = mk(role=role)
            segs.append(wrap(path, [rec(s, 1, T, 2, 1), rec(s, 2, T, 2, 1, rt=T + 1), rec(s, 1, T, 2, 1)], s, T))
            s = mk(role=role)
            segs.append(wrap(path, [rec(s, 1, T, 2, 1)], s, T))
            claims |= {f"C.nonleader_stepdown.{name}.{path}", f"C.nonleader_ignored.{name}.{path}"}
        # success and failure; NEED_MORE on both sides of nextIndex == last + 1
        s = mk()
        segs.append(wrap(path, [rec(s, 1, T, 2, 7), rec(s, 2, T, 2, 8), ], s, T))            # next = 10, 11
        s = mk()
        segs.append(wrap(path, [rec(s, 1, T, 2, 0, ok=0, ci=10), rec(s, 2, T, 2, 0, ok=0, ci=11)], s, T))
        claims |= {f"C.success.{path}", f"C.fail.{path}", f"C.need_more.set_at_last.{path}",
                   f"C.need_more.clear_at_last1.{path}"}
        # one peer repeated: the second reply's prev must match the updated nextIndex; the old one no longer does
        s = mk()
        segs.append(wrap(path, [rec(s, 1, T, 2, 3), rec(s, 1, T, 5, 2), rec(s, 1, T, 2, 3),
                                rec(s, 1, T, 7, 0, ok=0, ci=4), rec(s, 1, T, 3, 1)], s, T))
        # matchIndex moving down gives no range (peer 2 holds the quorum at 8, commit 8)
        s = gs.add(log, T=T, commit=8, match={1: 9, 2: 8}, nxt={1: 5, 2: 9})
        segs.append(wrap(path, [rec(s, 1, T, 4, 2)], s, T))
        claims |= {f"C.repeat.prev_updated.{path}", f"C.repeat.stale_prev.{path}", f"C.match_down.{path}"}
    # step-down at replies 63 and 64 of a long segment: the role carries across the batch edge
    for k in (63, 64):
        s = mk()
        body = [rec(s, 1, T, 2, 0)] * k + [rec(s, 2, T, 2, 0, rt=T + 1)] + [rec(s, 1, T, 2, 4), rec(s, 2, T, 2, 4)] * 2
        if k == 63:
            body[10] = rec(s, 2, T, 2, 2)      # an a1 range before it, so the commit of batch 0 stands
        segs.append(body)
        claims.add(f"C.stepdown.k{k}.long")
    items, sb = batch(segs)
    return len(gs.rows), P, L, gs.state(), items, sb, claims


def fam_quorum(P):
    """D: the order statistic at P: decided by a tie, the leader's own
    matchIndex entry above and below all others, quorum above last (clipped),
    quorum at or below the running H (no range)."""
    L, T = 16, 5
    gs = Groups(P, L)
    segs, claims = [], set()
    log = [T - 1] * 3 + [T] * 7                 # last = 10
    h = P // 2
    pre = f"D.P{P}."
    for path in ("group", "long"):
        for me in (0, P - 1, P // 2):
            oth = [j for j in range(P) if j != me]
            # tie: h - 1 peers already at 7, the reply brings one more to 7; the rest at 2
            if P >= 3:
                m = {j: (7 if i < h - 1 else 2) for i, j in enumerate(oth)}
                if h == 1:
                    m[oth[1]] = 7                  # P = 3: the other voter already at 7
                m[me] = 9
                s = gs.add(log, T=T, me=me, commit=2, match=m, head=me + 1)
                p = oth[h - 1] if h > 1 else oth[0]
                segs.append(wrap(path, [rec(s, p, T, m[p], 7 - m[p])], s, T, peer=oth[0]))
            # the leader's own entry above all others: would lift the quorum if counted
            m = {j: 2 for j in oth}
            m[me] = 10
            s = gs.add(log, T=T, me=me, commit=2, match=m, head=me + 2)
            body = [rec(s, j, T, 2, 4 + i) for i, j in enumerate(oth[:h])]
            segs.append(wrap(path, body, s, T, peer=oth[0]))
            # ... and below all others
            m = {j: 4 for j in oth}
            m[me] = 0
            s = gs.add(log, T=T, me=me, commit=3, match=m, nxt={j: 5 for j in oth}, head=me + 3)
            body = [rec(s, j, T, 4, 2 + i) for i, j in enumerate(oth[:h])]
            segs.append(wrap(path, body, s, T, peer=oth[0]))
            # clipped: the quorum acknowledges past last; then one at or below H: no range
            m = {j: 2 for j in oth}
            s = gs.add(log, T=T, me=me, commit=2, match=m, head=me + 4)
            body = [rec(s, j, T, 2, 11 + i) for i, j in enumerate(oth[:h])]
            body.append(rec(s, oth[0], T, 13, 0))
            segs.append(wrap(path, body, s, T, peer=oth[-1]))
    claims |= {pre + "self_high", pre + "self_low", pre + "clipped", pre + "no_range", pre + "no_range.group",
               pre + "no_range.long"}
    if P >= 3:
        claims |= {pre + "tie", pre + "tie.group", pre + "tie.long"}
    items, sb = batch(segs)
    return len(gs.rows), P, L, gs.state(), items, sb, claims


def fam_ranges():
    """E: the classes of an a1 range, two and three ranges in one segment with
    COMMITTED per reply, commitIndex == dummyIndex > 0, currentTerm 2^31 - 1,
    and a group at the top of the Index domain; L = 16."""
    P, L, T = 3, 16, 5
    gs = Groups(P, L)
    segs, claims = [], set()
    for path in ("group", "long"):
        E = f"E.{path}."
        pre = 5 if path == "long" else 0
        # probe hit over a longer range; settled by sorted terms; sorted with the top above currentTerm
        s = gs.add([3, 3, 4, 5, 5, 5, 6], T=T, commit=1, match={1: 1, 2: 1}, head=9)
        segs.append(wrap(path, [rec(s, 1, T, 1, 4)], s, T, pre))                   # (1, 5]: probe hit at 5
        s = gs.add([3, 3, 4, 4, 4, 4], T=T, commit=1, match={1: 1, 2: 1}, head=13)
        segs.append(wrap(path, [rec(s, 1, T, 1, 4)], s, T, pre))                   # top term 4 < 5, sorted: settled
        s = gs.add([3, 3, 4, 5, 6, 6, 6], T=T, commit=1, match={1: 1, 2: 1}, head=14)
        segs.append(wrap(path, [rec(s, 1, T, 1, 5)], s, T, pre))                   # top term 6 > 5: scan, hit at 4
        s = gs.add([5, 3, 3, 4, 4, 4, 4], T=T, commit=2, match={1: 2, 2: 2}, head=11)
        segs.append(wrap(path, [rec(s, 1, T, 2, 4)], s, T, pre))                   # unsorted, top below: scan, miss
        claims |= {E + "probe_hit", E + "settled", E + "sorted_top_above.scan_hit", E + "unsorted_top_below.scan"}
        # commitIndex == dummyIndex > 0, the dummy's own term currentTerm (must not be found)
        s = gs.add([4, 4, 4, 4, 6], T=T, dummy=7, dterm=T, commit=7, match={1: 7, 2: 7}, head=12)
        segs.append(wrap(path, [rec(s, 1, T, 7, 5)], s, T, pre))
        claims |= {E + "commit_eq_dummy", E + "term_at_commit", E + "wraps"}
        # two and three ranges in one segment (peer 1 and 2 alternate, each raising the quorum)
        log = [4, 4, 5, 4, 4, 6, 4, 5, 4, 6, 4, 4]       # Index 1..12; currentTerm at 3 and 8; unsorted
        mk = lambda h: gs.add(log, T=T, commit=1, match={1: 1, 2: 1}, head=h)  # noqa: E731
        s = mk(1)     # (1,3]: probe hit at 3; (3,6]: scan 4..5 miss
        segs.append(wrap(path, [rec(s, 1, T, 1, 2), rec(s, 2, T, 1, 5)], s, T, pre))
        s = gs.add(log, T=T, commit=3, match={1: 3, 2: 3}, head=2)   # (3,5]: scan 4, miss; (5,8]: probe hit at 8
        segs.append(wrap(path, [rec(s, 1, T, 3, 2), rec(s, 2, T, 3, 5)], s, T, pre))
        s = mk(3)     # (1,3]: probe hit; (3,10]: scan 4..9, hit at 8 (found in the tail launch on the group path)
        segs.append(wrap(path, [rec(s, 1, T, 1, 2), rec(s, 2, T, 1, 9), rec(s, 1, T, 3, 9)], s, T, pre))
        s = gs.add([4, 4, 5, 4, 4, 5, 4, 4, 6, 4], T=T, commit=1, match={1: 1, 2: 1}, head=4)
        segs.append(wrap(path, [rec(s, 1, T, 1, 3), rec(s, 2, T, 1, 6)], s, T, pre))   # (1,4]: hit 3; (4,7]: hit 6
        claims |= {E + "multi.probehit_scanmiss", E + "multi.scanmiss_probehit", E + "multi.probehit_scanhit",
                   E + "multi.scanhit_scanhit", E + "ranges2", E + "ranges3"}
        # currentTerm 2^31 - 1 in a scanning group (the scan's padding value is currentTerm + 1)
        s = gs.add([IMAX, IMAX, IMAX - 1, IMAX, IMAX - 1, IMAX - 1, IMAX - 1], T=IMAX, commit=2,
                   match={1: 2, 2: 2}, head=10)
        segs.append(wrap(path, [rec(s, 1, IMAX, 2, 4), rec(s, 2, IMAX, 2, 5)], s, IMAX, pre))
        claims.add(E + "term_max")
        # the group's Indexes at the top of the domain: last == 2^31 - 2
        d = TOP - 9
        s = gs.add([4, T, T, 4, T, 4, 4, 4, 4], T=T, dummy=d, dterm=3, commit=d + 2,
                   match={1: d + 2, 2: d + 2}, head=8)
        segs.append(wrap(path, [rec(s, 1, T, d + 2, 5), rec(s, 2, T, d + 2, 7)], s, T, pre))
        claims |= {E + "index_top", "B.idx_top_ok." + path}
    items, sb = batch(segs)
    return len(gs.rows), P, L, gs.state(), items, sb, claims


def fam_two_waves():
    """E: one k_fold wave (8 segments) whose pending list is ordered by lane:
    three ranges of segments 0-2, then two scan hits of segment 3, so the pair
    is scanned by different k_fold_tail waves (4 ranges each)."""
    P, L, T = 3, 16, 5
    gs = Groups(P, L)
    log = [4, 4, 5, 4, 4, 5, 4, 4, 6, 4]                  # currentTerm at 3 and 6
    segs = []
    for j in range(8):
        s = gs.add(log, T=T, commit=1, match={1: 1, 2: 1}, head=2 * j + 1)
        if j == 3:
            segs.append([rec(s, 1, T, 1, 3), rec(s, 2, T, 1, 6), rec(s, 1, T, 4, 4)])   # (1,4] hit 3; (4,8] hit 6
        else:
            segs.append([rec(s, 1, T, 1, 3)])                                        # (1,4]: scan, hit at 3
    items, sb = batch(segs)
    return 8, P, L, gs.state(), items, sb, {"E.group.multi.scanhit_scanhit", "E.group.multi.scanhit_scanhit.two_waves",
                                            "A.nseg8", "A.waves1"}


NSEG = (1, 7, 8, 9, 15, 16, 17, 53, 61, 69, 117, 125, 133, 197)    # waves 1, 2, 3, 7, 8, 9, 15, 16, 17, 25
FAMILIES = ([("lengths", fam_lengths, ())] + [(f"nseg{n}", fam_nseg, (n,)) for n in NSEG] +
            [("null", fam_null, ()), ("uncovered", fam_uncovered, ()), ("longpos", fam_longpos, ()),
             ("pending", fam_pending, ()), ("reject", fam_reject, ()), ("p1", fam_p1, ()), ("a2", fam_a2, ())] +
            [(f"quorum{P}", fam_quorum, (P,)) for P in range(2, 9)] +
            [("ranges", fam_ranges, ()), ("two_waves", fam_two_waves, ()),
             ("scan2048", fam_scan, (2048,)), ("scan1541", fam_scan, (1541,))])
SCAN_FAMILIES = ("ranges", "two_waves", "scan2048", "scan1541")
_cache = {}


def family(name):
    """(G, P, L, state, items, seg_begin, claims) of a family, built once; callers must not modify it."""
    if name not in _cache:
        fn, args = next((f, a) for n, f, a in FAMILIES if n == name)
        _cache[name] = fn(*args)
    return _cache[name]


def leader_peers(st, G, P):
    """Per group the replica that is Leader in `st` (-1: none)."""
    role = st["state"].reshape(G, P)
    return np.where((role == LEADER).any(axis=1), (role == LEADER).argmax(axis=1), -1).astype(np.int32)


def followup(name, st1, G, P, L, lp):
    """A second batch for the same engine: seeded reply segments of up to 12
    replies (both paths) on the state the first call left."""
    from oracle_lib import random_reply_segments
    seed = 9100 + [n for n, _, _ in FAMILIES].index(name)
    return random_reply_segments(st1, G, P, lp, seed=seed, max_len=12)


def run_family(name, engine_cls, oracle_cls, check_state):
    """The family on an engine against the oracle: flags, item errors and the
    whole state after the call, and after a follow-up batch. Returns n_items."""
    G, P, L, st, items, seg, _ = family(name)
    lp = leader_peers(st, G, P)
    o = oracle_cls(G, P, L, st)
    with engine_cls(G, P, L) as e:
        e.load_state(st)
        for call in range(2):
            if call:
                items, seg = followup(name, o.state(), G, P, L, lp)
            f, err = e.process_append_replies(items, seg)
            of, oerr = o.process_append_replies(items, seg)
            assert np.array_equal(err, oerr), f"{name} call {call}: item errors differ at {np.nonzero(err != oerr)[0][:8]}"
            assert np.array_equal(f, of), f"{name} call {call}: flags differ at {np.nonzero(f != of)[0][:8]}"
            check_state(e.store_state(), o.state(), G, P, L, f"{name} call {call}")
    return len(family(name)[4])


def main():
    from oracle_lib import Oracle, assert_states_equal

    from multiraft_amd import Engine
    return run_all([(n,) for n, _, _ in FAMILIES], lambda n: run_family(n, Engine, Oracle, assert_states_equal),
                   lambda n: len(family(n)[4]))


if __name__ == "__main__":
    sys.exit(main())
