"""Directed cases of the item-level kernels behind the C ABI
(multiraft_amd/csrc/mraft_kernels.hip): Snapshot, the InstallSnapshot gather,
HandleInstallSnapshot, processInstallSnapshotReply (raft_snapshot.go:3-69,
raft_append_entry.go:27-34), persistence (raft.go:205-235) and Start
(raft.go:90-104), shared by tests/test_snapshot_matrix.py (CPU: the model below
against the C oracle, and every claimed cell present in the model's
classification) and tests/test_snapshot_matrix_gpu.py (the engine against the
oracle, bit for bit; a child process runs this file on the small-grid library,
multiraft_amd/libmraft_hip_grid1.so). tests/snapshot_cases.py keeps the random
scenario; this file holds the chosen states.

Hand-built states: `Reps` places every replica of every group by hand (log,
ring head, dummy, commit, role, leader view, dirty bits). A family is a
function returning (G, P, L, state, batch, claims); `batch` is a dict of that
family's call inputs. `Model` restates each call in plain Python from the
oracle's statement, with the oracle's method names, and records per item its
class and ring positions in `Model.trace`; `cells` turns that record into cell
names, and `claims` must be among them. A family's calls are one script
(`SCRIPTS[kind]`) that runs unchanged on the model, the oracle and the engine
and returns every output in order; two runs agree when the outputs and the
final states do. Every script ends with a follow-up batch on the same engine,
so the slot claims' epoch is used a second time.

The cross-path families build whole groups (a leader and its followers) and
compare the two device statements of InstallSnapshot and of its reply rule:
the message-level calls in the tick's order (reach_model.masked_tick on the
engine) and mraft_replicate_tick in every mode, both against the oracle.

Cell names: see `cells`.

Run as a program: every family on the library MRAFT_LIB names against the
oracle, one JSON line {"cases": [[name, n_items, ok], ...]}, exit status 1 on
any mismatch."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from cases_program import run_all, sorted_terms  # noqa: E402

from multiraft_amd import _abi  # noqa: E402
from multiraft_amd._abi import (AE_ARGS, AE_ENTRIES_SORTED, CANDIDATE, E_INVAL, F_APPLIED,  # noqa: E402
                                F_SNAPSHOT_INSTALLED, F_STEPPED_DOWN, FOLLOWER, G_FOLLOWER_PANIC,
                                G_NEED_SNAPSHOT, G_SNAPSHOT_INSTALLED, G_STEPPED_DOWN, IS_ARGS, IS_REPLY, IS_RESULT,
                                ITEM_BAD_SLOT, ITEM_BAD_STATE, ITEM_BELOW_DUMMY, ITEM_DUP_SLOT, ITEM_LOG_FULL,
                                ITEM_NEED_SNAPSHOT, ITEM_PREV_BEYOND_LAST, LEADER, PERSISTENT, TICK_AUTO, TICK_FULL,
                                TICK_LIGHT, ptr)
from multiraft_amd.engine import copy_state, new_state  # noqa: E402

TOP = 2**31 - 2             # the highest Index of the engine's domain
IMAX = 2**31 - 1
KCHUNK = 256                # terms per iteration of wave_copy / wave_copy_from_ring (mraft_device.h kChunk)
ROLE = {LEADER: "leader", CANDIDATE: "candidate", FOLLOWER: "follower"}
ROW_LENS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)      # and L: terms of a persisted row
WRAPS = (0, 1, 63, 255, 256, 257)   # the row's term that sits at ring position 0 (0: head 0, no wrap)
DESCENTS = ((1, 2), (63, 64), (64, 65), (255, 256), (256, 257), (511, 512))   # the last: the row's last pair


# ---------------------------------------------------------------- states
class Reps:
    """Groups of P replicas, each placed by hand; the rest stay as Make left them."""

    def __init__(self, P: int, L: int):
        self.P, self.L, self.groups = P, L, []

    def group(self) -> int:
        self.groups.append({})
        return len(self.groups) - 1

    def put(self, g, p, log=(), T=5, role=FOLLOWER, dummy=0, dterm=0, head=0, commit=None, applied=None, voted=-1,
            match=None, nxt=None, hsnap=0, dirty=0, votes=0) -> int:
        """log: the terms of Index dummy + 1 .. last. match / nxt: {peer: value}
        (default 0 and last + 1). Returns the slot."""
        log = [int(t) for t in log]
        assert len(log) <= self.L - 1 and 0 <= p < self.P
        commit = dummy if commit is None else commit
        self.groups[g][p] = dict(log=log, T=T, role=role, dummy=dummy, dterm=dterm, head=head % self.L, commit=commit,
                                 applied=min(commit, dummy) if applied is None else applied, voted=voted,
                                 match=dict(match or {}), nxt=dict(nxt or {}), hsnap=hsnap, dirty=dirty, votes=votes,
                                 last=dummy + len(log))
        return g * self.P + p

    def add(self, p=0, **kw) -> int:
        return self.put(self.group(), p, **kw)

    def state(self, G=None) -> dict:
        G = len(self.groups) if G is None else G
        P, L = self.P, self.L
        assert len(self.groups) <= G
        st = new_state(G, P, L)
        for g, grp in enumerate(self.groups):
            for p, r in grp.items():
                s = g * P + p
                st["current_term"][s], st["state"][s], st["voted_for"][s] = r["T"], r["role"], r["voted"]
                st["dummy_index"][s], st["last_index"][s] = r["dummy"], r["last"]
                st["commit_index"][s], st["last_applied"][s] = r["commit"], r["applied"]
                st["log_head"][s], st["has_snapshot"][s] = r["head"], r["hsnap"]
                st["persist_dirty"][s], st["granted_votes"][s] = r["dirty"], r["votes"]
                terms = np.array([r["dterm"]] + r["log"], np.int32)
                st["log_term"][s * L + (r["head"] + np.arange(len(terms))) % L] = terms
                for j in range(P):
                    st["match_index"][s * P + j] = r["match"].get(j, 0)
                    st["next_index"][s * P + j] = r["nxt"].get(j, r["last"] + 1 if r["role"] == LEADER else 0)
        st["terms_sorted"] = sorted_terms(st, G, P, L)
        return st


def is_items(recs):
    out = np.zeros(len(recs), IS_RESULT)
    for i, r in enumerate(recs):
        out[i] = r
    return out


def is_args(recs):
    out = np.zeros(len(recs), IS_ARGS)
    for i, r in enumerate(recs):
        out[i] = r
    return out


# ---------------------------------------------------------------- the model
class Model:
    """Each call as the oracle states it, on a copy of `st`; `trace` holds one
    record per item (and per segment, row and call where cells need it)."""

    def __init__(self, G, P, L, st):
        self.G, self.P, self.L = G, P, L
        self.st = copy_state(st)
        self.trace = []
        self._starts = 0

    def state(self):
        return self.st

    def store_state(self):
        return copy_state(self.st)

    def _pos(self, s, i):
        return s * self.L + (int(self.st["log_head"][s]) + i - int(self.st["dummy_index"][s])) % self.L

    def _claim(self, slots):
        gp = self.G * self.P
        err, first = np.zeros(len(slots), np.int32), {}
        for i, s in enumerate(slots):
            s = int(s)
            if not 0 <= s < gp:
                err[i] = ITEM_BAD_SLOT
            elif s in first:
                err[i] = ITEM_DUP_SLOT
            else:
                first[s] = i
        return err, first

    @staticmethod
    def _claim_cls(e, s):
        return ("slot_neg" if s < 0 else "slot_gp") if e == ITEM_BAD_SLOT else "dup"

    # ---- Snapshot (raft_snapshot.go:3-13)
    def snapshot(self, slots, index):
        st, L = self.st, self.L
        slots, index = np.asarray(slots, np.int32), np.asarray(index, np.int32)
        err, first = self._claim(slots)
        for i, (s, x) in enumerate(zip(slots.tolist(), index.tolist())):
            R = dict(op="snapshot", i=i, n=len(slots), slot=s, x=x, moved=False, L=L)
            self.trace.append(R)
            if err[i]:
                R["cls"] = self._claim_cls(err[i], s)
                if err[i] == ITEM_DUP_SLOT:
                    R["dup_diff"] = x != int(index[first[s]]) and int(err[first[s]]) == 0
                continue
            d, last, h = int(st["dummy_index"][s]), int(st["last_index"][s]), int(st["log_head"][s])
            R.update(d=d, last=last, head0=h, dirty0=int(st["persist_dirty"][s]))
            if x <= d:                                                    # :6-9
                R["cls"] = "below" if x < d else "eq_dummy"
            elif x > last:                                                # sliceFrom panics
                err[i], R["cls"] = ITEM_PREV_BEYOND_LAST, "beyond"
            else:
                R["cls"], R["moved"] = "move", True
                R["rel"] = {n for n, c in (("dummy1", x == d + 1), ("mid", d + 1 < x < last),
                                           ("eq_last", x == last)) if c}
                R["raw"] = h + (x - d)
                st["log_head"][s] = R["head1"] = (h + (x - d)) % L         # :10
                st["dummy_index"][s] = x
                st["persist_dirty"][s] |= 3                               # :12
                R["commit_below"] = int(st["commit_index"][s]) < x
                R["applied_below"] = int(st["last_applied"][s]) < x
            R["dirty1"] = int(st["persist_dirty"][s])
        return err

    # ---- appendOneRound's two branches (raft_append_entry.go:20-54)
    def _gather_pre(self, op, s, p):
        gp, P = self.G * self.P, self.P
        R = dict(op=op, slot=s, peer=p, cls=None)
        self.trace.append(R)
        if not 0 <= s < gp:
            R["cls"] = "slot_neg" if s < 0 else "slot_gp"
        elif p < 0 or p >= P or p == s % P:
            R["cls"] = "peer_neg" if p < 0 else "peer_P" if p >= P else "peer_me"
        elif self.st["state"][s] != LEADER:
            R["cls"] = "role_" + ROLE[int(self.st["state"][s])]
        return R

    def gather_install_snapshot_args(self, slots, peers):
        st, P, L = self.st, self.P, self.L
        n = len(slots)
        out, err = np.zeros(n, IS_ARGS), np.zeros(n, np.int32)
        out["slot"] = -1
        for i, (s, p) in enumerate(zip(np.asarray(slots).tolist(), np.asarray(peers).tolist())):
            R = self._gather_pre("gather_is", s, p)
            R["i"] = i
            if R["cls"]:
                err[i] = ITEM_BAD_STATE if R["cls"].startswith("role_") else ITEM_BAD_SLOT
                continue
            nx, d, h = int(st["next_index"][s * P + p]), int(st["dummy_index"][s]), int(st["log_head"][s])
            R.update(next=nx, prev_rel=nx - 1 - d, head=h, L=L)
            if nx - 1 >= d:
                R["cls"] = "ae_due"
                continue
            R["cls"] = "args"
            out[i] = ((s // P) * P + p, int(st["current_term"][s]), s % P, d, int(st["log_term"][s * L + h]))
        return out, err

    def gather_append_args(self, slots, peers):
        st, P, L = self.st, self.P, self.L
        n = len(slots)
        out, err = np.zeros(n, AE_ARGS), np.zeros(n, np.int32)
        for i, (s, p) in enumerate(zip(np.asarray(slots).tolist(), np.asarray(peers).tolist())):
            R = self._gather_pre("gather_ae", s, p)
            R["i"] = i
            if R["cls"]:
                err[i] = ITEM_BAD_STATE if R["cls"].startswith("role_") else ITEM_BAD_SLOT
                continue
            d, last = int(st["dummy_index"][s]), int(st["last_index"][s])
            prev = int(st["next_index"][s * P + p]) - 1                     # :26
            if prev < d:
                err[i], R["cls"] = ITEM_NEED_SNAPSHOT, "need_snapshot"    # :27
            elif prev > last:
                err[i], R["cls"] = ITEM_PREV_BEYOND_LAST, "beyond"        # :41-43
            else:
                R["cls"] = "args"
                pt = int(st["log_term"][self._pos(s, prev)])
                srt = bool(st["terms_sorted"][s]) and (prev > d or prev == last or
                                                       pt <= int(st["log_term"][self._pos(s, prev + 1)]))
                out[i] = ((s // P) * P + p, int(st["current_term"][s]), s % P, prev, pt, int(st["commit_index"][s]),
                          last - prev, AE_ENTRIES_SORTED if srt else 0, s * L + (prev + 1 - d))
        return out, err

    # ---- HandleInstallSnapshot (raft_snapshot.go:15-54)
    def handle_install_snapshot(self, args, err_in=None):
        st, L = self.st, self.L
        args = np.ascontiguousarray(args, IS_ARGS)
        n = len(args)
        rep, fl = np.zeros(n, IS_REPLY), np.zeros(n, np.int32)
        err, first = self._claim(args["slot"])
        for i in range(n):
            a = args[i]
            f, at = int(a["slot"]), int(a["term"])
            lii, lit = int(a["last_included_index"]), int(a["last_included_term"])
            R = dict(op="handle", i=i, slot=f, lii=lii, incoming=bool(err_in is not None and err_in[i]), cls=None,
                     installed=False, L=L)
            self.trace.append(R)
            if err[i]:
                R["cls"] = self._claim_cls(err[i], f)
                continue
            if lii > TOP:                                                 # past the Index domain: malformed
                err[i], R["cls"] = ITEM_BAD_SLOT, "lii_domain"
                continue
            t, role0, commit = int(st["current_term"][f]), int(st["state"][f]), int(st["commit_index"][f])
            d, last, h = int(st["dummy_index"][f]), int(st["last_index"][f]), int(st["log_head"][f])
            R.update(tcmp="lt" if at < t else "eq" if at == t else "gt", role0=ROLE[role0],
                     srt0=int(st["terms_sorted"][f]),
                     voted0=int(st["voted_for"][f]), dirty0=int(st["persist_dirty"][f]), commit_below_dummy=commit < d,
                     rel={n_ for n_, c in (("eq_commit", lii == commit), ("commit1", lii == commit + 1),
                                           ("eq_last", lii == last), ("last1", lii == last + 1)) if c})
            if at >= t and commit < lii <= last and lii < d:              # sliceFrom panics
                err[i], R["cls"] = ITEM_BELOW_DUMMY, "below_dummy"
                continue
            if at < t:                                                    # :20-22
                rep[i] = (t, 0)
                R["cls"] = "stale_term"
                continue
            if at > t:                                                    # :23-26
                st["current_term"][f], st["voted_for"][f] = at, -1
                st["persist_dirty"][f] |= 1
            st["state"][f] = FOLLOWER                                     # :28
            rep[i] = (at, 0)
            if lii <= commit:                                             # :31-33
                R["cls"] = "outdated"
            else:
                R["installed"] = True
                if lii > last:                                            # :35-37
                    at_pos = f * L + h
                    R["cls"], R["head1"] = "new_log", h
                    st["last_index"][f], st["terms_sorted"][f] = lii, 1
                else:                                                     # :38-40
                    R["cls"], R["raw"], R["slice0"] = "slice", h + (lii - d), lii == d
                    R["head1"] = st["log_head"][f] = (h + (lii - d)) % L
                    at_pos = f * L + int(R["head1"])
                R["lit_differs"] = int(st["log_term"][at_pos]) != lit
                st["log_term"][at_pos] = lit                              # :44-45
                st["dummy_index"][f] = st["commit_index"][f] = st["last_applied"][f] = lii   # :42-43
                st["persist_dirty"][f] |= 3                               # :47
                st["has_snapshot"][f] = 1                                 # :52
                fl[i] = F_SNAPSHOT_INSTALLED
            R.update(voted1=int(st["voted_for"][f]), srt1=int(st["terms_sorted"][f]),
                     dirty_add=int(st["persist_dirty"][f]) & ~R["dirty0"], hsnap=int(st["has_snapshot"][f]))
        return rep, fl, err

    # ---- processInstallSnapshotReply (raft_snapshot.go:56-69)
    def process_install_snapshot_replies(self, items, seg_begin=None):
        st, P = self.st, self.P
        items = np.ascontiguousarray(items, IS_RESULT)
        n, gp = len(items), self.G * self.P
        ns = n if seg_begin is None else len(seg_begin) - 1
        fl, err = np.zeros(n, np.int32), np.zeros(n, np.int32)
        bounds = [(i, i + 1) if seg_begin is None else (int(seg_begin[i]), int(seg_begin[i + 1])) for i in range(ns)]
        owner = {}
        for sg, (b, e) in enumerate(bounds):
            if b < e and 0 <= b < n and 0 <= int(items["slot"][b]) < gp:
                owner.setdefault(int(items["slot"][b]), sg)
        self.trace.append(dict(op="fold_call", ns=ns, null=seg_begin is None))
        for sg, (b, e) in enumerate(bounds):
            S = dict(op="fold_seg", sg=sg, n=max(0, e - b), why=None, at=None, P=P, live=False)
            self.trace.append(S)
            if b >= e:
                continue
            slot = int(items["slot"][b])
            bad = 0
            if not 0 <= slot < gp:
                bad, S["why"] = ITEM_BAD_SLOT, "first_slot_oob"
            elif owner[slot] != sg:
                bad, S["why"] = ITEM_DUP_SLOT, "dup"
            else:
                for k in range(e - b):
                    r = items[b + k]
                    why = ("other_slot" if int(r["slot"]) != slot else "peer_neg" if r["peer"] < 0 else
                           "peer_P" if r["peer"] >= P else "peer_me" if r["peer"] == slot % P else
                           "lii" if int(r["args_last_included_index"]) > TOP else None)
                    if why:
                        bad = ITEM_BAD_SLOT
                        if S["why"] is None:
                            S["why"], S["at"] = why, k
            before = self._slot_image(slot) if 0 <= slot < gp else None
            if bad:
                err[b:e] = bad
                if before is not None:
                    S["stepdown_in"] = bool((items["reply_term"][b:e] > int(st["current_term"][slot])).any())
                continue
            t0, role0 = int(st["current_term"][slot]), int(st["state"][slot])
            S["role0"] = ROLE[role0]
            steps, seen = 0, set()
            for k in range(e - b):
                r = items[b + k]
                p, at, rt = int(r["peer"]), int(r["args_term"]), int(r["reply_term"])
                lii = int(r["args_last_included_index"])
                term, role = int(st["current_term"][slot]), int(st["state"][slot])
                R = dict(op="fold", sg=sg, k=k, n=e - b, after_stepdown=steps > 0, role0=ROLE[role0],
                         looks_ok=role0 == LEADER and at == t0 and rt <= t0, repeat=p in seen, kind=None)
                self.trace.append(R)
                seen.add(p)
                if rt > term:                                             # :59-64
                    st["current_term"][slot], st["voted_for"][slot], st["state"][slot] = rt, -1, FOLLOWER
                    st["persist_dirty"][slot] |= 1
                    fl[b + k] = F_STEPPED_DOWN
                    steps += 1
                    R["kind"], R["nth"] = "stepdown", steps
                elif role == LEADER and at == term:                       # :65-68
                    R.update(kind="applied", rcmp="eq" if rt == term else "lt", lii_top=lii == TOP,
                             lowers=lii < int(st["match_index"][slot * P + p]) and
                             lii + 1 < int(st["next_index"][slot * P + p]))
                    st["match_index"][slot * P + p], st["next_index"][slot * P + p] = lii, lii + 1
                    fl[b + k] = F_APPLIED
                else:
                    R["kind"] = "nonleader" if role != LEADER else "args_below" if at < term else "args_above"
            S["live"] = bool(fl[b:e].any())
            S["unchanged"] = before == self._slot_image(slot)
        return fl, err

    def _slot_image(self, s):
        st, P = self.st, self.P
        return tuple(int(st[k][s]) for k in ("current_term", "voted_for", "state", "persist_dirty", "commit_index")) + \
            tuple(st["match_index"][s * P:(s + 1) * P].tolist()) + tuple(st["next_index"][s * P:(s + 1) * P].tolist())

    # ---- Start (raft.go:90-104) and the applier (raft.go:153-203)
    def start(self, slots, counts=None):
        st, L = self.st, self.L
        slots = np.asarray(slots, np.int32)
        n = len(slots)
        idx, term, isl = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        err, first = self._claim(slots)
        self._starts += 1
        for i, s in enumerate(slots.tolist()):
            k = 1 if counts is None else int(counts[i])
            R = dict(op="start", i=i, slot=s, k=k, null_counts=counts is None, cls=None, call=self._starts)
            self.trace.append(R)
            if err[i]:
                R["cls"] = self._claim_cls(err[i], s)
                if err[i] == ITEM_DUP_SLOT:
                    R["dup_diff"] = counts is not None and k != int(counts[first[s]])
                continue
            if k < 1:
                err[i], R["cls"] = ITEM_BAD_SLOT, "count_lt1"
                continue
            if st["state"][s] != LEADER:                                  # :93-95
                R["cls"] = "not_leader"
                continue
            last, d, T = int(st["last_index"][s]), int(st["dummy_index"][s]), int(st["current_term"][s])
            if last + k - d > L - 1 or last + k > TOP:
                err[i], R["cls"] = ITEM_LOG_FULL, "log_full"
                continue
            R.update(cls="appended", srt0=int(st["terms_sorted"][s]),
                     top_cmp=None if last == d else "above" if int(st["log_term"][self._pos(s, last)]) > T else
                     "eq" if int(st["log_term"][self._pos(s, last)]) == T else "below")
            if R["top_cmp"] == "above":
                st["terms_sorted"][s] = 0
            pos = [self._pos(s, last + j) - s * L for j in range(1, k + 1)]
            R["pos"], R["srt1"] = pos, int(st["terms_sorted"][s])
            for q in pos:
                st["log_term"][s * L + q] = T                             # :96-100
            st["last_index"][s] = last + k
            st["persist_dirty"][s] |= 1                                   # :101
            idx[i], term[i], isl[i] = last + 1, T, 1
        return idx, term, isl, err

    def collect_apply(self, snapshots=False):
        st, gp = self.st, self.G * self.P
        fr, to = np.zeros(gp, np.int32), np.zeros(gp, np.int32)
        si, stm = np.zeros(gp, np.int32), np.zeros(gp, np.int32)
        for s in range(gp):
            if snapshots:
                hs = st["has_snapshot"][s] != 0
                si[s] = st["dummy_index"][s] if hs else -1
                stm[s] = st["log_term"][s * self.L + st["log_head"][s]] if hs else 0
                st["has_snapshot"][s] = 0
            fr[s], to[s] = st["last_applied"][s] + 1, st["commit_index"][s]
            if to[s] > st["last_applied"][s]:
                st["last_applied"][s] = to[s]
        return (fr, to, si, stm) if snapshots else (fr, to)

    # ---- persistence (raft.go:205-235)
    def collect_persist(self):
        out = self.st["persist_dirty"].copy()
        self.st["persist_dirty"][:] = 0
        return out

    def read_persistent_raw(self, slots, cap):
        st, L = self.st, self.L
        hdr = np.zeros(len(slots), PERSISTENT)
        off, seen = 0, set()
        call = dict(op="read_call", n=len(slots), order=[int(s) for s in slots], twice=False, cap_short=False)
        self.trace.append(call)
        for i, s in enumerate(np.asarray(slots).tolist()):
            d, last = int(st["dummy_index"][s]), int(st["last_index"][s])
            hdr[i] = (s, int(st["current_term"][s]), int(st["voted_for"][s]), d, last, 0, off)
            off += last - d + 1
            call["twice"] |= s in seen
            seen.add(s)
        if cap < off:
            call["cap_short"] = cap == off - 1
            return E_INVAL, hdr, np.zeros(0, np.int32)
        terms = np.zeros(off, np.int32)
        for i, s in enumerate(np.asarray(slots).tolist()):
            cnt, h = int(hdr["last_index"][i] - hdr["dummy_index"][i]) + 1, int(st["log_head"][s])
            o = int(hdr["terms_offset"][i])
            terms[o:o + cnt] = st["log_term"][s * L + (h + np.arange(cnt)) % L]
            # w: the row's term at ring position 0 (0: the head itself)
            self.trace.append(dict(op="read_row", cnt=cnt, head=h, w=(L - h) % L, L=L))
        return 0, hdr, terms

    def restore(self, hdr, terms):
        st, P, L = self.st, self.P, self.L
        hdr = np.ascontiguousarray(hdr, PERSISTENT)
        gp, nt = self.G * P, len(terms)
        err, seen = np.zeros(len(hdr), np.int32), set()
        for i, r in enumerate(hdr):
            s, d, last, off = int(r["slot"]), int(r["dummy_index"]), int(r["last_index"]), int(r["terms_offset"])
            cnt = last - d + 1
            R = dict(op="restore", i=i, slot=s, cnt=cnt, L=L, cls=None)
            self.trace.append(R)
            why = ("slot_neg" if s < 0 else "slot_gp" if s >= gp else "last_lt_dummy" if cnt < 1 else
                   "dummy_neg" if d < 0 else "off_neg" if off < 0 else "off_past" if off + cnt > nt else None)
            if why:
                err[i], R["cls"] = ITEM_BAD_SLOT, why
            elif cnt > L:
                err[i], R["cls"] = ITEM_LOG_FULL, "too_long"
            elif s in seen:
                err[i], R["cls"] = ITEM_DUP_SLOT, "dup"
            if err[i]:
                continue
            seen.add(s)
            R["cls"] = "restored"
            R["was"] = dict(role=ROLE[int(st["state"][s])], head=int(st["log_head"][s]),
                            hsnap=int(st["has_snapshot"][s]),
                            dirty=int(st["persist_dirty"][s]), votes=int(st["granted_votes"][s]),
                            view=bool(st["match_index"][s * P:(s + 1) * P].any() and
                                      st["next_index"][s * P:(s + 1) * P].any()))
            row = np.asarray(terms[off:off + cnt], np.int64)
            R["descents"] = [int(k) for k in np.nonzero(row[:-1] > row[1:])[0]]     # pair (k, k + 1)
            st["state"][s], st["current_term"][s], st["voted_for"][s] = FOLLOWER, r["current_term"], r["voted_for"]
            st["log_term"][s * L:s * L + cnt] = terms[off:off + cnt]
            st["log_head"][s] = st["has_snapshot"][s] = st["granted_votes"][s] = st["persist_dirty"][s] = 0
            st["dummy_index"][s] = st["commit_index"][s] = st["last_applied"][s] = d
            st["last_index"][s] = last
            st["terms_sorted"][s] = R["srt"] = int(not [k for k in R["descents"] if k >= 1])
            st["match_index"][s * P:(s + 1) * P] = 0
            st["next_index"][s * P:(s + 1) * P] = 0
        return err


# ---------------------------------------------------------------- script steps per kind of object
def handle_is_prefilled(eng, args, err_in):
    """HandleInstallSnapshot with the caller's item_err array as it stands
    (out=; allocated outputs are zeros): (replies, flags, item_err)."""
    if isinstance(eng, Model):
        return eng.handle_install_snapshot(args, err_in)
    n = len(args)
    return eng.handle_install_snapshot(args, out=(np.zeros(n, IS_REPLY), np.zeros(n, np.int32),
                                                  np.array(err_in, np.int32)))


def read_persistent_raw(eng, slots, cap):
    """mraft_read_persistent with a chosen terms_cap, raw because the rc of a
    cap one short is an output: (rc, headers, terms)."""
    if isinstance(eng, Model):
        return eng.read_persistent_raw(slots, cap)
    slots = np.ascontiguousarray(slots, np.int32)
    n = len(slots)
    hdr, terms = np.zeros(n, PERSISTENT), np.zeros(max(cap, 1), np.int32)
    if hasattr(eng, "_h"):
        rc = _abi.lib().mraft_read_persistent(eng._h, ptr(slots), n, ptr(hdr), ptr(terms), cap)
    else:
        import oracle_lib
        rc = oracle_lib.lib().ora_read_persistent(ctypes.byref(eng._e), ptr(slots), n, ptr(hdr), ptr(terms), cap)
    used = int((hdr["last_index"].astype(np.int64) - hdr["dummy_index"] + 1).sum())
    return rc, hdr, (terms[:used].copy() if rc == 0 else np.zeros(0, np.int32))


def compact_of(eng, snapshots):
    """collect_apply_compact as (slots, snap_index, snap_term, from, to, total);
    for the oracle and the model derived from collect_apply, whose slots with a
    message are the compacted list."""
    if hasattr(eng, "collect_apply_compact"):
        out = eng.collect_apply_compact(snapshots=snapshots)
        if snapshots:
            return out
        sl, fr, to, n = out
        return sl, np.zeros(0, np.int32), np.zeros(0, np.int32), fr, to, n
    # without the snapshot outputs only commitIndex > lastApplied counts, and only the listed slots advance
    if snapshots:
        fr, to, si, stm = eng.collect_apply(snapshots=True)
        sel = np.nonzero((to >= fr) | (si >= 0))[0]
        return sel.astype(np.int32), si[sel], stm[sel], fr[sel], to[sel], len(sel)
    fr, to = eng.collect_apply()
    sel = np.nonzero(to >= fr)[0]
    return sel.astype(np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), fr[sel], to[sel], len(sel)


def tick_of(eng, lp):
    """One full tick where the object has one (the model has none)."""
    return [np.asarray(eng.replicate_tick(lp))] if hasattr(eng, "replicate_tick") else []


# ---------------------------------------------------------------- scripts
def _clip(a):
    return np.minimum(np.asarray(a, np.int64), IMAX).astype(np.int32)


def followup_snapshot(b):
    """The second batch of a snapshot family: the slots in reverse order, one Index up."""
    return b["slots"][::-1].copy(), _clip(b["index"][::-1].astype(np.int64) + 1)


def followup_handle(b):
    """... of a handle family: the args in reverse order, newer terms, one Index up."""
    a2 = b["args"][::-1].copy()
    a2["term"] += 1
    a2["last_included_index"] = _clip(a2["last_included_index"].astype(np.int64) + 1)
    return a2


def followup_fold(b):
    """... of a fold family: the segments in reverse order, args_term raised to
    a higher reply_term (what the stepped-down replicas now hold)."""
    items, seg = b["items"], b["seg"]
    if seg is None:
        items2, seg2 = items[::-1].copy(), None
    else:
        parts = [items[int(x):int(y)] for x, y in zip(seg[:-1], seg[1:])][::-1]
        items2 = np.concatenate(parts).copy() if parts else items[:0].copy()
        seg2 = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    items2["args_term"] = np.maximum(items2["reply_term"], items2["args_term"])
    return items2, seg2


def image(eng):
    """The whole state as an output of a script: compared with
    assert_states_equal (ring heads included) wherever a script takes it, so
    nothing a later call overwrites goes unseen."""
    return eng.store_state()


def script_snapshot(eng, b, tick=True):
    out = [eng.snapshot(b["slots"], b["index"]), image(eng)]
    out.append(eng.collect_persist())
    if tick and "lp" in b:
        out += tick_of(eng, b["lp"]) + [image(eng)]
    out += [eng.snapshot(*followup_snapshot(b)), image(eng)]
    out.append(eng.collect_persist())
    return out


def script_gather(eng, b, tick=True):
    out = []
    for sl, pr in ((b["slots"], b["peers"]), (b["slots"][::-1], b["peers"][::-1])):
        out += list(eng.gather_install_snapshot_args(sl, pr))
        out += list(eng.gather_append_args(sl, pr))
        out.append(image(eng))                                             # the gathers change nothing
    return out


def script_handle(eng, b, tick=True):
    """The batch, the applier without the snapshot outputs, then the compacted
    one with them, twice each; the follow-up; the applier with them."""
    out = list(handle_is_prefilled(eng, b["args"], b["err_in"])) + [image(eng)]
    out += list(eng.collect_apply()) + list(eng.collect_apply()) + [image(eng)]
    out += list(compact_of(eng, True)) + list(compact_of(eng, True)) + [image(eng)]
    out += list(eng.handle_install_snapshot(followup_handle(b))) + [image(eng)]
    out += list(eng.collect_apply(snapshots=True)) + list(eng.collect_apply(snapshots=True))
    out += list(compact_of(eng, False))
    out.append(eng.collect_persist())
    return out


def script_handle_snap(eng, b, tick=True):
    """The same batch on an engine of its own, the appliers the other way
    round: mraft_collect_apply with the snapshot outputs straight after the
    batch, twice, then without them; after the follow-up the compacted one."""
    out = list(handle_is_prefilled(eng, b["args"], b["err_in"])) + [image(eng)]
    out += list(eng.collect_apply(snapshots=True)) + list(eng.collect_apply(snapshots=True)) + [image(eng)]
    out += list(eng.collect_apply()) + list(eng.collect_apply())
    out += list(eng.handle_install_snapshot(followup_handle(b))) + [image(eng)]
    out += list(compact_of(eng, True)) + list(compact_of(eng, True)) + [image(eng)]
    out.append(eng.collect_persist())
    return out


def script_fold(eng, b, tick=True):
    out = list(eng.process_install_snapshot_replies(b["items"], b["seg"])) + [image(eng)]
    out.append(eng.collect_persist())
    out += list(eng.process_install_snapshot_replies(*followup_fold(b))) + [image(eng)]
    out.append(eng.collect_persist())
    return out


def script_persist(eng, b, tick=True):
    rc, hdr, terms = read_persistent_raw(eng, b["slots"], b["need"])
    out = [np.int64(rc), hdr, terms]
    rc2, hdr2, _ = read_persistent_raw(eng, b["slots"], b["need"] - 1)     # terms_cap one short
    out += [np.int64(rc2), hdr2, image(eng)]                               # a read-out changes nothing
    out.append(eng.collect_persist())
    out += [eng.restore(hdr, terms), image(eng)]                           # restore(read_persistent(x))
    if tick:
        out += tick_of(eng, b["lp"]) + [image(eng)]                        # the leaders left out of it replicate
    rc3, hdr3, terms3 = read_persistent_raw(eng, b["slots"][::-1], b["need"])
    out += [np.int64(rc3), hdr3, terms3, eng.collect_persist()]
    return out


def script_restore(eng, b, tick=True):
    out = [eng.restore(b["hdr"], b["terms"]), image(eng), eng.collect_persist()]
    if tick:
        out += tick_of(eng, b["lp"]) + [image(eng)]
    out += [eng.restore(b["hdr"][::-1], b["terms"]), image(eng), eng.collect_persist()]
    return out


def script_start(eng, b, tick=True):
    out = list(eng.start(b["slots"], b["counts"])) + [image(eng)]
    out += list(eng.start(b["slots_null"], None)) + [image(eng)]
    out.append(eng.collect_persist())
    out += list(eng.start(b["slots"][::-1], b["counts"][::-1])) + [image(eng)]
    out.append(eng.collect_persist())
    return out


def script_grid(eng, b, tick=True):
    out = [image(eng)]                                                     # k_terms_sorted ran at load
    out += list(eng.collect_apply(snapshots=True)) + [image(eng), eng.collect_persist(), image(eng)]
    out += list(eng.collect_apply()) + [eng.collect_persist()]
    return out


SCRIPTS = dict(snapshot=script_snapshot, gather=script_gather, handle=script_handle, handle_snap=script_handle_snap,
               fold=script_fold, persist=script_persist, restore=script_restore, start=script_start, grid=script_grid)


# ---------------------------------------------------------------- cells
def cells(trace) -> set:
    """The matrix cells a run contains, from the model's record.

    S (Snapshot): S.idx.<below|eq_dummy|dummy1|mid|eq_last|beyond|last_top>, S.head.<Lm1|zero_exact|past_wrap>,
       S.commit_below_dummy, S.applied_below_dummy, S.persist.moved3, S.persist.unmoved0, S.dup.first_wins_other_index,
       S.slot.<neg|gp>, S.batch_gt256, S.pos255, S.pos256
    G (gather): G.prev.dummy_m1, G.prev.eq_dummy, G.next0, G.role.<follower|candidate>, G.peer.<me|P|neg>,
       G.slot.<neg|gp>, G.dterm.<head0|mid|Lm1>, G.need_snapshot_iff_args
    H (handle): H.term.<lt|eq|gt>.<follower|candidate|leader>, H.lii.<eq_commit|commit1|eq_last|last1|top|past_domain>,
       H.below_dummy, H.below_dummy.newer_term, H.slice0, H.head.<Lm1|zero_exact|past_wrap>, H.lit_differs,
       H.voted.<reset_gt|kept_eq>, H.hsnap, H.persist.<0|1|3>, H.srt.<new_log_sets|slice_keeps0|slice_keeps1>,
       H.dup, H.slot.<neg|gp>, H.incoming_err
    F (reply fold): F.null_seg_begin, F.explicit, F.len0, F.len1, F.lenPm1, F.len_gtPm1, F.applied,
       F.stepdown.<first|middle|last>, F.stepdown.second_higher, F.after_stepdown_ignored, F.reply_eq_term,
       F.reply_below_term, F.args_below.leader, F.args_above.leader, F.nonleader_ignored.<follower|candidate>,
       F.lowers_match_next, F.bad.<peer_me|peer_neg|peer_P|other_slot|lii.k0|lii.klast>, F.bad.stepdown_inside,
       F.first_slot_oob, F.dup_later, F.lii.top, F.nseg_gt64, F.seg<63|64|65>
    P (persistence): P.read.n<cnt>.w<w> (a row of cnt terms whose term w sits at ring position 0; w0: head 0),
       P.read.iter2 / P.read.wrap_in_iter2 (wave_copy_from_ring's second iteration, a wrap inside it),
       P.read.unordered, P.read.slot_twice, P.read.cap_short, P.restore.descent.<a>_<b>, P.restore.descent.last,
       P.restore.descent.0_1_sorted, P.restore.sorted, P.restore.iter2, P.restore.resets_all, P.accept.L_terms,
       P.refuse.<slot_neg|slot_gp|last_lt_dummy|dummy_neg|off_neg|off_past|too_long|dup>
    T (Start): T.dup_other_count, T.counts_null, T.count0, T.cross.<first|middle|last>, T.top_above_clears,
       T.top_eq_keeps"""
    out = set()
    tr = list(trace)
    # ---- S
    first_call = [R for R in tr if R["op"] == "snapshot"]
    if first_call:
        n0 = first_call[0]["n"]
        snaps = first_call[:n0]                       # the family's batch; the follow-up's records come after
        for R in snaps:
            c = R["cls"]
            if c in ("below", "eq_dummy", "beyond"):
                out.add("S.idx." + c)
                if R["dirty1"] == R["dirty0"] == 0:
                    out.add("S.persist.unmoved0")
            elif c == "move":
                out |= {"S.idx." + r for r in R["rel"]}
                if R["last"] == TOP:
                    out.add("S.idx.last_top")
                L_ = R["raw"] - R["head1"]            # 0 or L
                if R["head1"] == 0 and L_:
                    out.add("S.head.zero_exact")
                elif L_:
                    out.add("S.head.past_wrap")
                elif R["head1"] == R["L"] - 1:
                    out.add("S.head.Lm1")
                if R["commit_below"]:
                    out.add("S.commit_below_dummy")
                if R["applied_below"]:
                    out.add("S.applied_below_dummy")
                if R["dirty0"] == 0 and R["dirty1"] == 3:
                    out.add("S.persist.moved3")
                if R["i"] in (255, 256):
                    out.add(f"S.pos{R['i']}")
            elif c == "dup" and R["dup_diff"]:
                out.add("S.dup.first_wins_other_index")
            elif c in ("slot_neg", "slot_gp"):
                out.add("S.slot." + c[5:])
        if n0 > 256:
            out.add("S.batch_gt256")
    # ---- G
    gi = [R for R in tr if R["op"] == "gather_is"]
    ga = [R for R in tr if R["op"] == "gather_ae"]
    if gi:
        half = len(gi) // 2                           # the script gathers the batch, then its reverse
        for R in gi[:half]:
            c = R["cls"]
            if c == "args":
                if R["prev_rel"] == -1:
                    out.add("G.prev.dummy_m1")
                if R["next"] == 0:
                    out.add("G.next0")
                out.add("G.dterm." + ("head0" if R["head"] == 0 else "Lm1" if R["head"] == R["L"] - 1 else "mid"))
            elif c == "ae_due" and R["prev_rel"] == 0:
                out.add("G.prev.eq_dummy")
            elif c.startswith("role_"):
                out.add("G.role." + c[5:])
            elif c.startswith("peer_"):
                out.add("G.peer." + c[5:])
            elif c.startswith("slot_"):
                out.add("G.slot." + c[5:])
        pairs = list(zip(gi[:half], ga[:half]))
        if pairs and all((a["cls"] == "args") == (b_["cls"] == "need_snapshot") for a, b_ in pairs) \
                and any(a["cls"] == "args" for a, _ in pairs) and any(a["cls"] == "ae_due" for a, _ in pairs):
            out.add("G.need_snapshot_iff_args")
    # ---- H
    hs = [R for R in tr if R["op"] == "handle"]
    if hs:
        n0 = max(R["i"] for R in hs) + 1
        for R in hs[:n0]:
            c = R["cls"]
            if R["incoming"] and R["installed"]:
                out.add("H.incoming_err")
            if c == "dup":
                out.add("H.dup")
            elif c in ("slot_neg", "slot_gp"):
                out.add("H.slot." + c[5:])
            elif c == "lii_domain":
                out.add("H.lii.past_domain")
            if "tcmp" not in R:
                continue
            if c == "below_dummy":
                out.add("H.below_dummy.newer_term" if R["tcmp"] == "gt" else "H.below_dummy")
                continue
            out.add(f"H.term.{R['tcmp']}.{R['role0']}")
            if c == "stale_term":
                continue
            out |= {"H.lii." + r for r in R["rel"]}
            out.add(f"H.persist.{R['dirty_add']}")
            if R["tcmp"] == "gt" and R["voted0"] != -1 and R["voted1"] == -1:
                out.add("H.voted.reset_gt")
            if R["tcmp"] == "eq" and R["voted0"] != -1 and R["voted1"] == R["voted0"]:
                out.add("H.voted.kept_eq")
            if not R["installed"]:
                continue
            if R["hsnap"]:
                out.add("H.hsnap")
            if R["lii"] == TOP:
                out.add("H.lii.top")
            if R["lit_differs"]:
                out.add("H.lit_differs")
            if c == "new_log" and R["srt0"] == 0 and R["srt1"] == 1:
                out.add("H.srt.new_log_sets")
            if c == "slice":
                out.add(f"H.srt.slice_keeps{R['srt0']}" if R["srt1"] == R["srt0"] else "H.srt.slice_changes")
                if R["slice0"] and R["commit_below_dummy"]:
                    out.add("H.slice0")
                L_ = R["raw"] - R["head1"]
                if R["head1"] == 0 and L_:
                    out.add("H.head.zero_exact")
                elif L_:
                    out.add("H.head.past_wrap")
                elif R["head1"] == R["L"] - 1:
                    out.add("H.head.Lm1")
    # ---- F
    calls = [R for R in tr if R["op"] == "fold_call"]
    if calls:
        c0 = calls[0]
        out.add("F.null_seg_begin" if c0["null"] else "F.explicit")
        at = [i for i, R in enumerate(tr) if R["op"] == "fold_call"] + [len(tr)]
        first = tr[at[0]:at[1]]
        segs = [R for R in first if R["op"] == "fold_seg"]
        reps = [R for R in first if R["op"] == "fold"]
        if c0["ns"] > 64:
            out.add("F.nseg_gt64")
        for S in segs:
            P = S["P"]
            if S["why"] is None:
                if not c0["null"]:
                    out.add("F.len0" if S["n"] == 0 else "F.len1" if S["n"] == 1 else "F.lenPm1" if S["n"] == P - 1
                            else "F.len_gtPm1" if S["n"] > P - 1 else "F.len_other")
                    if S["n"] == 1 and P == 2:
                        out.add("F.lenPm1")
                if S["sg"] in (63, 64, 65) and S["live"]:
                    out.add(f"F.seg{S['sg']}")
                if S["n"] and S["role0"] != "leader" and S["unchanged"] and \
                        any(R["sg"] == S["sg"] and R["kind"] == "nonleader" for R in reps):
                    out.add(f"F.nonleader_ignored.{S['role0']}")
            elif S["why"] == "dup":
                out.add("F.dup_later")
            elif S["why"] == "first_slot_oob":
                out.add("F.first_slot_oob")
            elif S["why"] == "lii":
                out.add("F.bad.lii." + ("k0" if S["at"] == 0 else "klast" if S["at"] == S["n"] - 1 else "kmid"))
            else:
                out.add("F.bad." + S["why"])
            if S["why"] and S.get("stepdown_in"):
                out.add("F.bad.stepdown_inside")
        for R in reps:
            k = R["kind"]
            if k == "stepdown":
                if R["nth"] == 1:
                    out.add("F.stepdown." + ("first" if R["k"] == 0 else "last" if R["k"] == R["n"] - 1 else "middle"))
                else:
                    out.add("F.stepdown.second_higher")
            elif k == "applied":
                out.add("F.applied")
                out.add("F.reply_eq_term" if R["rcmp"] == "eq" else "F.reply_below_term")
                if R["lowers"]:
                    out.add("F.lowers_match_next")
                if R["lii_top"]:
                    out.add("F.lii.top")
                if R["repeat"]:
                    out.add("F.repeat_peer")
            elif k in ("args_below", "args_above") and not R["after_stepdown"]:
                out.add(f"F.{k}.leader")
            elif k == "nonleader" and R["after_stepdown"] and R["looks_ok"]:
                out.add("F.after_stepdown_ignored")
    # ---- P
    rc = [R for R in tr if R["op"] == "read_call"]
    if rc:
        c0 = rc[0]
        if c0["twice"]:
            out.add("P.read.slot_twice")
        if c0["order"] != sorted(c0["order"]) and c0["order"] != sorted(c0["order"], reverse=True):
            out.add("P.read.unordered")
        if len(rc) > 1 and rc[1]["cap_short"]:
            out.add("P.read.cap_short")
        at = [i for i, R in enumerate(tr) if R["op"] == "read_call"] + [len(tr)]
        for R in tr[at[0]:at[1]]:
            if R["op"] != "read_row":
                continue
            name = "L" if R["cnt"] == R["L"] else str(R["cnt"])
            out.add(f"P.read.n{name}.w{R['w']}")
            if R["cnt"] > KCHUNK:
                out.add("P.read.iter2")
                if KCHUNK <= R["w"] < R["cnt"]:
                    out.add("P.read.wrap_in_iter2")
    rs = [R for R in tr if R["op"] == "restore"]
    if rs:
        n0 = max(R["i"] for R in rs) + 1
        for R in rs[:n0]:
            c = R["cls"]
            if c != "restored":
                out.add("P.refuse." + c)
                continue
            if R["cnt"] == R["L"]:
                out.add("P.accept.L_terms")
            if R["cnt"] > KCHUNK:
                out.add("P.restore.iter2")
            d = R["descents"]
            if not d:
                out.add("P.restore.sorted")
            elif len(d) == 1:
                k = d[0]
                if k == 0 and R["srt"] == 1:
                    out.add("P.restore.descent.0_1_sorted")
                elif R["srt"] == 0:
                    out.add(f"P.restore.descent.{k}_{k + 1}")
                    if k == R["cnt"] - 2:
                        out.add("P.restore.descent.last")
            w = R["was"]
            if w["role"] == "leader" and w["head"] and w["hsnap"] and w["dirty"] and w["votes"] and w["view"]:
                out.add("P.restore.resets_all")
    # ---- T
    for R in (R for R in tr if R["op"] == "start" and R["call"] <= 2):   # the batch and the NULL-counts call
        c = R["cls"]
        if R["null_counts"] and c == "appended":
            out.add("T.counts_null")
        if c == "dup" and R["dup_diff"]:
            out.add("T.dup_other_count")
        if c == "count_lt1" and R["k"] == 0:
            out.add("T.count0")
        if c == "appended":
            if R["k"] >= 3 and 0 in R["pos"]:
                j = R["pos"].index(0)
                out.add("T.cross." + ("first" if j == 0 else "last" if j == R["k"] - 1 else "middle"))
            if R["top_cmp"] == "above" and R["srt0"] == 1 and R["srt1"] == 0:
                out.add("T.top_above_clears")
            if R["top_cmp"] == "eq" and R["srt0"] == R["srt1"] == 1:
                out.add("T.top_eq_keeps")
    return out


# ---------------------------------------------------------------- families
BASE = [3, 3, 4, 4, 5, 5, 5, 5]           # a follower's or leader's log after its dummy: sorted, ends at currentTerm 5


def fam_snapshot(P, L, big=False):
    """Snapshot: the Index against the log, the new head against the ring's
    end, the reference's quirk (commitIndex and lastApplied stay below the new
    dummy) at a leader that then ticks, duplicate and out-of-range slots; with
    `big`, 290 items with the two wrapping ones at positions 255 and 256."""
    rp = Reps(P, L)
    it, claims = [], set()

    def one(x_rel, head=2, dummy=4, cell=None, **kw):
        s = rp.add(log=BASE, dummy=dummy, dterm=2, head=head, commit=dummy, **kw)
        it.append((s, dummy + x_rel))
        if cell:
            claims.add(cell)
        return s

    one(-2, cell="S.idx.below"); one(0, cell="S.idx.eq_dummy"); one(1, cell="S.idx.dummy1")
    one(4, cell="S.idx.mid"); one(8, cell="S.idx.eq_last"); one(9, cell="S.idx.beyond")
    one(8, dummy=TOP - 8, head=5)
    one(5, dummy=TOP - 8, head=7)
    claims.add("S.idx.last_top")
    one(3, head=L - 4, cell="S.head.Lm1")
    wrap = [one(3, head=L - 3, cell="S.head.zero_exact"), one(3, head=L - 1, cell="S.head.past_wrap")]
    wrap_items = it[-2:]
    # the quirk at a leader: commit and lastApplied stay below the new dummy; its group ticks
    g = rp.group()
    lead = rp.put(g, 0, log=BASE, role=LEADER, dummy=4, dterm=2, head=3, commit=5, applied=5,
                  match={j: 5 for j in range(1, P)}, nxt={j: 6 for j in range(1, P)})
    for j in range(1, P):
        rp.put(g, j, log=BASE[:4], dummy=4, dterm=2, commit=5, applied=5)
    it.append((lead, 8))
    claims |= {"S.commit_below_dummy", "S.applied_below_dummy", "S.persist.moved3", "S.persist.unmoved0"}
    s = one(2)
    it.append((s, 7))                      # the later item of the slot asks for another Index
    claims.add("S.dup.first_wins_other_index")
    it += [(-1, 3), (None, 3)]
    claims |= {"S.slot.neg", "S.slot.gp"}
    G = len(rp.groups)
    if big:
        it = [x for x in it if x not in wrap_items]
        fill = []
        while len(fill) + len(it) + 2 < 290:
            s = rp.put(rp.group() if len(fill) % P == 0 else len(rp.groups) - 1, len(fill) % P, log=BASE, dummy=4,
                       dterm=2, head=len(fill) % L, commit=4)
            fill.append((s, 5 + len(fill) % 7))
        it = fill[:255] + wrap_items + fill[255:] + it
        assert it[255][0] == wrap[0] and it[256][0] == wrap[1]
        claims |= {"S.batch_gt256", "S.pos255", "S.pos256"}
        G = len(rp.groups)
    assert G <= 64
    gp = G * P
    slots = np.array([gp if s is None else s for s, _ in it], np.int32)
    lp = np.full(G, -1, np.int32)
    lp[g] = 0
    batch = dict(slots=slots, index=np.array([x for _, x in it], np.int32), lp=lp, quirk_group=g)
    return G, P, L, rp.state(G), batch, claims


def fam_gather(P, L):
    """The InstallSnapshot gather beside the AppendEntries gather on the same
    items: next - 1 on both sides of the dummy, next == 0, non-leaders, bad
    peers and slots, dummyTerm read at three ring positions."""
    rp = Reps(P, L)
    it, claims = [], set()
    peer = 1
    for head, cell in ((0, "head0"), (L // 2, "mid"), (L - 1, "Lm1")):
        s = rp.add(p=0, log=BASE, role=LEADER, dummy=6, dterm=9 + head % 5, head=head, commit=7, nxt={peer: 6})
        it.append((s, peer))                                             # next - 1 == dummy - 1: args
        claims.add("G.dterm." + cell)
    s = rp.add(p=P - 1, log=BASE, role=LEADER, dummy=6, dterm=2, head=4, commit=7, nxt={0: 7})
    it.append((s, 0))                                                    # next - 1 == dummy: an AppendEntries is due
    s = rp.add(p=0, log=BASE, role=LEADER, dummy=3, dterm=2, head=5, commit=3, nxt={peer: 0})
    it.append((s, peer))                                                 # next == 0
    s = rp.add(p=0, log=BASE, role=LEADER, dummy=6, dterm=2, head=1, commit=7, nxt={peer: 14})
    it.append((s, peer))                                                 # the last entry: a heartbeat
    claims |= {"G.prev.dummy_m1", "G.prev.eq_dummy", "G.next0"}
    for role in (FOLLOWER, CANDIDATE):
        s = rp.add(p=0, log=BASE, role=role, dummy=6, dterm=2, nxt={peer: 3})
        it.append((s, peer))
        claims.add("G.role." + ROLE[role])
    s = rp.add(p=0, log=BASE, role=LEADER, dummy=6, dterm=2, nxt={j: 3 for j in range(P)})
    it += [(s, 0), (s, P), (s, -1), (-1, peer), (None, peer)]
    claims |= {"G.peer.me", "G.peer.P", "G.peer.neg", "G.slot.neg", "G.slot.gp", "G.need_snapshot_iff_args"}
    G = len(rp.groups)
    gp = G * P
    batch = dict(slots=np.array([gp if s is None else s for s, _ in it], np.int32),
                 peers=np.array([p for _, p in it], np.int32))
    return G, P, L, rp.state(), batch, claims


UNSORTED = [4, 2, 3, 3, 4, 4]


def fam_handle(P, L):
    """HandleInstallSnapshot: args.term against the follower's term for every
    role, LastIncludedIndex against commit, last and the dummy, the slice's
    head against the ring's end, the Index domain's top and the first Index
    past it, duplicate and out-of-range slots, an incoming item error."""
    rp = Reps(P, L)
    args, err_in, claims = [], [], set()
    T = 5

    def fol(at=T, lii=None, lit=9, log=BASE[:6], dummy=10, commit=12, head=3, role=FOLLOWER, voted=1, incoming=0, **kw):
        s = rp.add(p=len(args) % P, log=log, T=T, role=role, dummy=dummy, dterm=1, head=head, commit=commit,
                   applied=min(commit, dummy + 1), voted=voted, **kw)
        args.append((s, at, (s + 1) % P, commit + 1 if lii is None else lii, lit))
        err_in.append(incoming)
        return s

    for at, tc in ((T - 1, "lt"), (T, "eq"), (T + 2, "gt")):
        for role in (FOLLOWER, CANDIDATE, LEADER):
            fol(at=at, role=role, match={0: 3, 1: 4}, nxt={0: 4, 1: 5})
            claims.add(f"H.term.{tc}.{ROLE[role]}")
    fol(lii=12); fol(at=T + 1, lii=12); fol(lii=13); fol(lii=16); fol(lii=17)
    claims |= {"H.lii.eq_commit", "H.lii.commit1", "H.lii.eq_last", "H.lii.last1", "H.persist.0", "H.persist.1",
               "H.persist.3", "H.voted.reset_gt", "H.voted.kept_eq", "H.hsnap", "H.lit_differs"}
    fol(lii=8, commit=7); fol(at=T + 3, lii=8, commit=7)                  # commit < lii <= last, lii < dummy
    fol(lii=10, commit=7)                                               # a slice by zero
    claims |= {"H.below_dummy", "H.below_dummy.newer_term", "H.slice0"}
    for head, cell in ((L - 4, "Lm1"), (L - 3, "zero_exact"), (L - 1, "past_wrap")):
        fol(lii=13, head=head)
        claims.add("H.head." + cell)
    fol(lii=17, log=UNSORTED); fol(lii=11, log=UNSORTED, commit=10); fol(lii=14)
    claims |= {"H.srt.new_log_sets", "H.srt.slice_keeps0", "H.srt.slice_keeps1"}
    fol(lii=TOP); fol(lii=IMAX)
    fol(lii=TOP, log=BASE[:6], dummy=TOP - 6, commit=TOP - 3)            # the slice that ends at the top of the domain
    claims |= {"H.lii.top", "H.lii.past_domain"}
    s = fol(lii=13)
    args.append((s, T + 1, 0, 15, 8))                                    # the slot a second time
    err_in.append(0)
    fol(lii=14, incoming=ITEM_BAD_STATE)
    gp = len(rp.groups) * P
    args += [(-1, T, 0, 13, 9), (gp, T, 0, 13, 9)]
    err_in += [0, ITEM_DUP_SLOT]
    claims |= {"H.dup", "H.slot.neg", "H.slot.gp", "H.incoming_err"}
    batch = dict(args=is_args(args), err_in=np.array(err_in, np.int32))
    return len(rp.groups), P, L, rp.state(), batch, claims


def fam_fold(P, L, null=False):
    """processInstallSnapshotReply: the reply rule on chosen leaders and
    non-leaders, the segment prologue's rejections, and 70 segments with chosen
    ones at segment indexes 63, 64 and 65; with `null`, one item per segment
    and no seg_begin."""
    rp = Reps(P, L)
    T, D = 5, 6
    segs, claims = [], set()
    count = [0]

    def lead(role=LEADER, me=None, T_=T, match=2, nxt=3):
        k = count[0]
        count[0] += 1
        g = rp.group() if k % P == 0 else len(rp.groups) - 1
        me = k % P
        return rp.put(g, me, log=BASE, T=T_, role=role, dummy=D, dterm=2, head=k % L, commit=7, voted=me,
                      match={j: match for j in range(P) if j != me}, nxt={j: nxt for j in range(P) if j != me})

    def peers(s):
        return [j for j in range(P) if j != s % P]

    def r(s, k=0, at=T, lii=D, rt=T, peer=None):
        return (s, peers(s)[k % (P - 1)] if peer is None else peer, at, lii, rt)

    def live():
        s = lead()
        return [r(s, count[0])]

    if null:
        s1, s2, s3, s4 = lead(), lead(), lead(role=FOLLOWER), lead()
        s5, s6, s7 = lead(), lead(), lead()
        recs = [r(s1), r(s2, rt=T + 1), r(s3), r(s4, at=T - 1), r(s1, 1), r(-1), r(s5, peer=s5 % P, rt=T + 1),
                r(s6, peer=P, rt=T + 1), r(s7, lii=IMAX, rt=T + 1)]
        claims = {"F.null_seg_begin", "F.applied", "F.stepdown.first", "F.nonleader_ignored.follower",
                  "F.args_below.leader", "F.dup_later", "F.first_slot_oob", "F.bad.peer_me", "F.bad.peer_P",
                  "F.bad.lii.k0", "F.bad.stepdown_inside"}
        return len(rp.groups), P, L, rp.state(), dict(items=is_items(recs), seg=None), claims
    # lengths 0, 1, P - 1 and beyond it (a peer repeated, the later reply's Index stands)
    s = lead()
    segs += [[], [r(s)]]
    s = lead()
    segs.append([r(s, k) for k in range(P - 1)])
    s = lead()
    segs.append([r(s, k, lii=D - (k >= P - 1)) for k in range(P + 1)])
    claims |= {"F.explicit", "F.len0", "F.len1", "F.lenPm1", "F.len_gtPm1", "F.applied", "F.reply_eq_term",
               "F.repeat_peer"}
    # step-down first, in the middle, last; a second one by a still higher term; what follows is ignored
    for where in ("first", "middle", "last"):
        s = lead()
        body = [r(s, 0), r(s, 1), r(s, 0), r(s, 1)]
        body.insert({"first": 0, "middle": 2, "last": 4}[where], r(s, 1, rt=T + 2))
        segs.append(body)
        claims.add("F.stepdown." + where)
    s = lead()
    segs.append([r(s, 0, rt=T + 1), r(s, 1), r(s, 0, rt=T + 4), r(s, 1, at=T + 4, rt=T + 4)])
    claims |= {"F.stepdown.second_higher", "F.after_stepdown_ignored"}
    # a reply of an older term still applies (:59 asks only for a higher one); stale and future args at a leader
    s = lead()
    segs.append([r(s, 0, rt=T - 2), r(s, 1, at=T - 1), r(s, 1, at=T + 1, rt=T)])
    claims |= {"F.reply_below_term", "F.args_below.leader", "F.args_above.leader"}
    for role in (FOLLOWER, CANDIDATE):
        s = lead(role=role)
        segs.append([r(s, 0), r(s, 1, rt=T - 1)])
        claims.add("F.nonleader_ignored." + ROLE[role])
    s = lead(match=9, nxt=10)
    segs.append([r(s, 0)])
    s = lead()
    segs.append([r(s, 0, lii=TOP)])
    claims |= {"F.lowers_match_next", "F.lii.top"}
    # rejections: the whole segment, a step-down reply inside it or not
    for why in ("peer_me", "peer_neg", "peer_P", "other_slot", "lii.k0", "lii.klast"):
        s = lead()
        body = [r(s, 0), r(s, 1, rt=T + 3), r(s, 0)]
        k = 0 if why == "lii.k0" else 2
        body[k] = {"peer_me": r(s, peer=s % P), "peer_neg": r(s, peer=-1), "peer_P": r(s, peer=P),
                   "other_slot": (s + P,) + r(s, 0)[1:], "lii.k0": r(s, 0, lii=IMAX),
                   "lii.klast": r(s, 0, lii=IMAX)}[why]
        segs.append(body)
        claims.add("F.bad." + why)
    claims.add("F.bad.stepdown_inside")
    segs.append([r(-1, 0)])
    sa = lead()
    segs += [[r(sa, 0)], live(), [r(sa, 1, rt=T + 1)]]
    claims |= {"F.first_slot_oob", "F.dup_later"}
    while len(segs) < 63:
        segs.append(live())
    s = lead()
    segs.append([r(s, 0), r(s, 1, rt=T + 1)])                          # 63: applies, then steps down
    s = lead()
    segs.append([r(s, 0, rt=T + 2)])                                   # 64
    s = lead()
    segs.append([r(s, k) for k in range(P - 1)])                        # 65
    while len(segs) < 70:
        segs.append(live())
    claims |= {"F.nseg_gt64", "F.seg63", "F.seg64", "F.seg65"}
    flat = [x for sgm in segs for x in sgm]
    seg = np.concatenate([[0], np.cumsum([len(sgm) for sgm in segs])]).astype(np.int64)
    assert len(rp.groups) <= 64
    return len(rp.groups), P, L, rp.state(), dict(items=is_items(flat), seg=seg), claims


def _row_terms(s, cnt):
    return ((np.arange(cnt) * 7 + s * 3) % 50 + 1).astype(np.int32)      # unsorted, distinct per slot


def fam_persist(P, L):
    """The read-out: rows of every length around the 64-lane and 256-term
    edges of wave_copy_from_ring, each with the ring's wrap at head 0, between
    terms 0 and 1, in the last lane of the first load, and on the 256-term
    boundary and one either side of it; the rows read in no order, one slot
    twice; terms_cap one short; then restore(read_persistent(x)) and a tick in
    which each group's leader, the one replica not restored, replicates to the
    restored followers."""
    rp = Reps(P, L)
    claims = set()
    slots = []
    k = 0
    R = P - 1                               # rows per group; its last replica is the leader the restore leaves out
    for cnt in ROW_LENS + (L,):
        for w in WRAPS:
            g = rp.group() if k % R == 0 else len(rp.groups) - 1
            s = g * P + k % R
            k += 1
            t = _row_terms(s, cnt)
            rp.put(g, s % P, log=t[1:], T=60 + s % 5, role=(FOLLOWER, CANDIDATE, LEADER)[s % 3], dummy=s % 4,
                   dterm=int(t[0]), head=(L - w) % L, commit=s % 4, voted=s % P, dirty=s % 4, hsnap=s % 2, votes=s % 3,
                   match={j: 1 for j in range(P)}, nxt={j: 2 for j in range(P)})
            slots.append(s)
            claims.add(f"P.read.n{'L' if cnt == L else cnt}.w{w}")
    # one leader per group, not read out and not restored: after the restore it sends each restored follower
    # the entries behind that follower's own last Index (or its own last), so the tick compares restored rows
    for g, grp in enumerate(rp.groups):
        nx = {p: min(r["last"], 300) + 1 for p, r in grp.items()}
        rp.put(g, P - 1, log=[70] * 300, T=70, role=LEADER, dummy=0, dterm=0, head=g % L, commit=0, voted=P - 1,
               match={j: 0 for j in range(P)}, nxt=nx)
    order = slots[1::2] + slots[0::2][::-1]
    order.insert(5, order[40])                                            # one slot named twice
    G = len(rp.groups)
    assert G <= 64
    st = rp.state()
    need = int(sum(int(st["last_index"][s] - st["dummy_index"][s]) + 1 for s in order))
    claims |= {"P.read.iter2", "P.read.wrap_in_iter2", "P.read.unordered", "P.read.slot_twice", "P.read.cap_short"}
    batch = dict(slots=np.array(order, np.int32), need=need, lp=np.full(G, P - 1, np.int32))
    return G, P, L, st, batch, claims


def fam_restore(P, L):
    """Restore: rows of 513 terms with one descent at each 64-pair edge of
    wave_terms_sorted, at the 256-term edge of wave_copy and at the last pair;
    a row of exactly L terms; every refusal, each aimed at a replica that was
    leader with a moved head, a pending snapshot, dirty bits and votes."""
    rp = Reps(P, L)
    claims = set()
    hdr, chunks = [], []
    off = [0]

    def dirty():
        k = sum(len(g) for g in rp.groups)
        g = rp.group() if k % P == 0 else len(rp.groups) - 1
        me = k % P
        return rp.put(g, me, log=BASE, T=9, role=LEADER, dummy=3, dterm=2, head=5 + k % 7, commit=6, applied=5,
                      voted=me, hsnap=1, dirty=1 + k % 3, votes=1 + k % 2, match={j: 4 for j in range(P)},
                      nxt={j: 5 for j in range(P)})

    def item(s, terms, dummy=20, T=7, voted=1, last=None, offset=None):
        terms = np.asarray(terms, np.int32)
        hdr.append((s, T, voted, dummy, dummy + len(terms) - 1 if last is None else last, 0,
                    off[0] if offset is None else offset))
        chunks.append(terms)
        off[0] += len(terms)

    def row(cnt, descent=None):
        t = np.full(cnt, 5, np.int32)
        if descent is not None:
            t[:descent + 1] = 8                      # 8 ... 8 5 ... 5: one descent, at (descent, descent + 1)
        else:
            t[cnt // 2:] = 6
        return t

    for a, b_ in DESCENTS:
        item(dirty(), row(513, a))
        claims.add(f"P.restore.descent.{a}_{b_}")
    item(dirty(), row(513, 0))                                           # only the dummy above its successor: sorted
    item(dirty(), row(300))
    item(dirty(), row(L, 100))                                           # exactly L terms
    claims |= {"P.restore.descent.last", "P.restore.descent.0_1_sorted", "P.restore.sorted", "P.restore.iter2",
               "P.restore.resets_all", "P.accept.L_terms"}
    first = dirty()
    item(first, row(3))
    # the refusals
    item(-1, row(2)); item(None, row(2))
    item(dirty(), row(2), last=19)                                       # last < dummy
    item(dirty(), row(2), dummy=-1)
    item(dirty(), row(2), offset=-1)
    item(dirty(), row(L + 1))                                            # L + 1 terms
    item(first, row(4, 1))                                               # a duplicate
    past = dirty()
    gp = len(rp.groups) * P
    total = off[0]
    item(past, row(2), offset=total - 1)                                 # offset + count past n_terms
    chunks.pop()
    claims |= {"P.refuse." + c for c in ("slot_neg", "slot_gp", "last_lt_dummy", "dummy_neg", "off_neg", "off_past",
                                         "too_long", "dup")}
    h = np.zeros(len(hdr), PERSISTENT)
    for i, x in enumerate(hdr):
        h[i] = (gp if x[0] is None else x[0],) + x[1:]
    G = len(rp.groups)
    return G, P, L, rp.state(), dict(hdr=h, terms=np.concatenate(chunks), lp=np.zeros(G, np.int32)), claims


def fam_start(P, L):
    """Start, beyond tests/light_cases.py: a duplicate slot asking for another
    count, counts NULL, a count of 0, a run of three entries whose first,
    second or third lands on ring position 0, and a last term above or equal
    to currentTerm."""
    rp = Reps(P, L)
    T = 5
    sl, cn, claims = [], [], set()
    for j, where in enumerate(("first", "middle", "last")):
        # last = dummy + 8 sits at head + 8; entry j + 1 of the run lands on 0
        s = rp.add(p=j % P, log=BASE, T=T, role=LEADER, dummy=2, dterm=1, head=(L - 9 - j) % L, commit=2)
        sl.append(s); cn.append(3)
        claims.add("T.cross." + where)
    s = rp.add(log=BASE[:4] + [7], T=T, role=LEADER, dummy=2, dterm=1, head=4)
    sl.append(s); cn.append(2)
    s = rp.add(log=BASE[:5], T=T, role=LEADER, dummy=2, dterm=1, head=6)
    sl.append(s); cn.append(1)
    claims |= {"T.top_above_clears", "T.top_eq_keeps"}
    s = rp.add(log=BASE[:3], T=T, role=LEADER, dummy=2, dterm=1, head=1)
    sl += [s, s]; cn += [2, 4]                                           # the first wins: two entries
    s = rp.add(log=BASE[:3], T=T, role=LEADER, dummy=2, dterm=1)
    sl.append(s); cn.append(0)
    s = rp.add(log=BASE[:3], T=T, role=FOLLOWER, dummy=2, dterm=1)
    sl.append(s); cn.append(1)
    nl = [rp.add(log=BASE[:2], T=T, role=LEADER, dummy=2, dterm=1, head=L - 3),
          rp.add(log=BASE[:2], T=T, role=CANDIDATE, dummy=2, dterm=1)]
    claims |= {"T.dup_other_count", "T.count0", "T.counts_null"}
    batch = dict(slots=np.array(sl, np.int32), counts=np.array(cn, np.int32), slots_null=np.array(nl, np.int32))
    return len(rp.groups), P, L, rp.state(), batch, claims


def fam_grid():
    """An engine of G * P = 300 slots for the four grid-stride loops: on the
    small-grid library k_init_state, k_collect_apply and k_collect_persist run
    a second pass (one workgroup covers 256 slots) and k_terms_sorted 75 passes
    (4 slots each); unsorted rows past slot 4, in both passes' ranges."""
    P, L = 5, 16
    rp = Reps(P, L)
    for g in range(60):
        rp.group()
        for p in range(P):
            s = g * P + p
            log = [3 + (k * (1 + s % 3)) % 4 if s % 3 == 0 else 3 + k // 2 for k in range(s % 9)]
            rp.put(g, p, log=log, T=7, role=(FOLLOWER, LEADER, CANDIDATE)[s % 3], dummy=s % 5, dterm=1, head=s % L,
                   commit=s % 5 + min(len(log), s % 4), applied=s % 5, hsnap=int(s % 7 == 0), dirty=s % 4)
    st = rp.state()
    uns = np.nonzero(st["terms_sorted"] == 0)[0]
    assert (uns > 4).all() and (uns < 256).any() and (uns >= 256).any()
    return 60, P, L, st, {}, set()


# ---------------------------------------------------------------- cross-path groups
def fam_cross(P, L):
    """Whole groups for the two device statements of InstallSnapshot and its
    reply rule (the message-level calls; the tick body): args.term the
    leader's term, LastIncludedIndex its dummy.
      mixed      peer 1 is due a snapshot (a new log), its neighbours AppendEntries
      stepdown   the snapshot reply of peer 1 carries a higher term; peer 2's AppendEntries succeeds
      panic      peer 1's sliceFrom would panic: commit < lii <= last, lii < its dummy
      slice      peer 1 installs by a slice whose head wraps; peer 2 is behind and appends
      masked     `mixed` again, run under a mask that disconnects peer 1"""
    rp = Reps(P, L)
    T, D = 5, 6
    names = ("mixed", "stepdown", "panic", "slice", "masked")
    for name in names:
        g = rp.group()
        nx = {j: 11 for j in range(1, P)}
        nx[1] = 3                                                        # next - 1 < dummy
        if name == "slice" and P > 2:
            nx[2] = 9
        rp.put(g, 0, log=BASE[:4], T=T, role=LEADER, dummy=D, dterm=3, head=L - 2, commit=8, applied=8, voted=0,
               match={j: 8 for j in range(1, P)}, nxt=nx)
        for j in range(1, P):
            rp.put(g, j, log=BASE[:4], T=T, dummy=D, dterm=3, head=j, commit=8, applied=8, voted=0)
        if name in ("mixed", "masked"):
            rp.put(g, 1, log=[1, 1], T=T - 1, dummy=0, dterm=0, head=L - 1, commit=1, applied=1, voted=0)
        elif name == "stepdown":
            rp.put(g, 1, log=[1, 1], T=T + 2, dummy=0, dterm=0, head=2, commit=1, applied=1, voted=1)
        elif name == "panic":
            rp.put(g, 1, log=[2, 2, 2, 2], T=T, dummy=8, dterm=2, head=3, commit=5, applied=5, voted=0)
        elif name == "slice":
            rp.put(g, 1, log=[1, 1, 2, 2, 3, 3, 4, 4], T=T, dummy=1, dterm=1, head=L - 3, commit=4, applied=4, voted=0)
            if P > 2:
                rp.put(g, 2, log=BASE[:2], T=T, dummy=D, dterm=3, head=L - 1, commit=7, applied=7, voted=0)
    G = len(names)
    reach = np.full(G, (1 << P) - 1, np.uint8)
    reach[names.index("masked")] &= ~np.uint8(2)
    claims = {"X.is_stepdown", "X.follower_panic", "X.slice_wraps", "X.masked_snapshot_dropped"}
    if P > 2:                               # a group of two has no neighbour due AppendEntries
        claims |= {"X.mixed", "X.is_stepdown_before_ae_success"}
    return G, P, L, rp.state(), dict(lp=np.zeros(G, np.int32), reach=reach, names=names), claims


class EngineAsOracle:
    """The engine with the oracle's attributes reach_model.masked_tick reads:
    G, P and `st`, whose every look is a fresh read-out of that array."""

    class _Live:
        def __init__(self, e):
            self.e = e

        def __getitem__(self, k):
            return self.e.scalar_state(fields=(k,))[k]

    def __init__(self, e):
        self.e, self.G, self.P = e, e.G, e.P
        self.st = self._Live(e)

    def __getattr__(self, name):
        return getattr(self.e, name)


def cross_expected(oracle_cls, name):
    """The oracle's answers for a cross-path family: the tick without a mask,
    the tick under the family's mask (composed from the oracle's message-level
    calls), and the record of that composition without a mask."""
    from reach_model import full_mask, masked_tick
    G, P, L, st, b, _ = family(name)
    o = oracle_cls(G, P, L, st)
    gf = o.replicate_tick(b["lp"])
    om = oracle_cls(G, P, L, st)
    gfm = masked_tick(om, b["lp"], b["reach"])
    oc = oracle_cls(G, P, L, st)
    rec = {}
    gfc = masked_tick(oc, b["lp"], full_mask(G, P), rec)
    return dict(plain=(gf, o.state()), masked=(gfm, om.state()), composed=(gfc, oc.state()), record=rec)


def cross_cells(name, exp) -> set:
    G, P, L, st, b, _ = family(name)
    gf, rec, names = exp["plain"][0], exp["record"], b["names"]
    gfm = exp["masked"][0]
    out = set()
    for g, nm in enumerate(names):
        snap, ae = rec["snap"][g], rec["ae"][g]
        if snap.any() and gf[g] & G_NEED_SNAPSHOT:
            if nm == "mixed" and gf[g] & G_SNAPSHOT_INSTALLED and ae.any():
                out.add("X.mixed")
            if gf[g] & G_STEPPED_DOWN and rec["reply_term_higher"][g][snap].any():
                out.add("X.is_stepdown")
                p = int(np.nonzero(snap)[0][0])
                if (rec["reply_success"][g][p + 1:] & ae[p + 1:]).any():
                    out.add("X.is_stepdown_before_ae_success")
            if gf[g] & G_FOLLOWER_PANIC:
                out.add("X.follower_panic")
            if nm == "slice" and gf[g] & G_SNAPSHOT_INSTALLED:
                f = g * P + 1
                if exp["plain"][1]["log_head"][f] < st["log_head"][f]:
                    out.add("X.slice_wraps")
            if nm == "masked" and gf[g] & G_SNAPSHOT_INSTALLED and not gfm[g] & G_SNAPSHOT_INSTALLED \
                    and gfm[g] & G_NEED_SNAPSHOT:
                out.add("X.masked_snapshot_dropped")
    return out


def run_cross(name, engine_cls, oracle_cls, check_state):
    """(a) the message-level calls in the tick's order on the engine and (b)
    mraft_replicate_tick in full mode with 1 and 2 shards, in light and in auto
    mode, without and under the family's mask: all against the oracle."""
    from reach_model import full_mask, masked_tick
    G, P, L, st, b, _ = family(name)
    exp = cross_expected(oracle_cls, name)
    with engine_cls(G, P, L) as e:
        e.load_state(st)
        gf = masked_tick(EngineAsOracle(e), b["lp"], full_mask(G, P))
        assert np.array_equal(gf, exp["plain"][0]), f"{name} message path: group flags {gf} vs {exp['plain'][0]}"
        check_state(e.store_state(), exp["plain"][1], G, P, L, f"{name} message path")
    for mode, shards in ((TICK_FULL, 1), (TICK_FULL, 2), (TICK_LIGHT, 1), (TICK_AUTO, 1)):
        for key, mask in (("plain", None), ("masked", b["reach"])):
            with engine_cls(G, P, L) as e:
                e.load_state(st)
                e.set_tick_mode(mode)
                e.set_tick_shards(shards)
                if mask is not None:
                    e.set_reachable(mask)
                gf = e.replicate_tick(b["lp"])
                ctx = f"{name} tick mode {mode} shards {shards} {key}"
                assert np.array_equal(gf, exp[key][0]), f"{ctx}: group flags {gf} vs {exp[key][0]}"
                check_state(e.store_state(), exp[key][1], G, P, L, ctx)
    return G * P


# ---------------------------------------------------------------- the list
FAMILIES = (
    [(f"snapshot{L}", "snapshot", fam_snapshot, (3, L)) for L in (16, 13)] +
    [("snapshot_big", "snapshot", fam_snapshot, (8, 13, True))] +
    [(f"gather{P}_{L}", "gather", fam_gather, (P, L)) for P, L in ((2, 16), (3, 13), (8, 16))] +
    [(f"handle{P}_{L}", "handle", fam_handle, (P, L)) for P, L in ((3, 16), (5, 13), (2, 13))] +
    [(f"handle{P}_{L}_snap", "handle_snap", fam_handle, (P, L)) for P, L in ((3, 16), (5, 13), (2, 13))] +
    [(f"fold{P}_{L}", "fold", fam_fold, (P, L)) for P, L in ((3, 16), (5, 13), (2, 16), (8, 13))] +
    [("fold_null", "fold", fam_fold, (3, 13, True))] +
    [(f"persist{L}", "persist", fam_persist, (3, L)) for L in (520, 515)] +
    [(f"restore{L}", "restore", fam_restore, (3, L)) for L in (520, 515)] +
    [(f"start{L}", "start", fam_start, (3, L)) for L in (16, 13)] +
    [("grid300", "grid", fam_grid, ())] +
    [(f"cross{P}_{L}", "cross", fam_cross, (P, L)) for P, L in ((3, 16), (5, 13), (2, 16), (8, 13))])
NAMES = [f[0] for f in FAMILIES]
KIND = {f[0]: f[1] for f in FAMILIES}
_cache = {}


def family(name):
    """(G, P, L, state, batch, claims) of a family, built once; callers must not modify it."""
    if name not in _cache:
        _, _, fn, args = next(f for f in FAMILIES if f[0] == name)
        _cache[name] = fn(*args)
    return _cache[name]


def n_items(name):
    b = family(name)[4]
    n = int(sum(len(v) for k, v in b.items() if k in ("slots", "args", "items", "hdr")))
    return n or family(name)[0] * family(name)[1]


def compare_outputs(got, want, ctx, check_state, dims):
    """Two runs of one script, output by output; a state image (a dict) by
    `check_state`, the suites' assert_states_equal."""
    assert len(got) == len(want), f"{ctx}: {len(got)} outputs vs {len(want)}"
    for k, (a, b_) in enumerate(zip(got, want)):
        if isinstance(a, dict):
            check_state(a, b_, *dims, f"{ctx}: the state at output {k}")
            continue
        a, b_ = np.asarray(a), np.asarray(b_)
        if a.dtype.names:
            for f in a.dtype.names:
                if f != "_pad" and not np.array_equal(a[f], b_[f]):
                    bad = np.nonzero(a[f] != b_[f])[0][:8]
                    raise AssertionError(f"{ctx}: output {k}.{f} differs at {bad}: {a[f][bad]} vs {b_[f][bad]}")
        elif a.shape != b_.shape or not np.array_equal(a, b_):
            bad = np.nonzero(a != b_)[0][:8] if a.shape == b_.shape else "shape"
            raise AssertionError(f"{ctx}: output {k} differs at {bad}: {a[bad] if a.shape == b_.shape else a.shape} vs "
                                 f"{b_[bad] if a.shape == b_.shape else b_.shape}")


def run_family(name, engine_cls, oracle_cls, check_state):
    """The family on an engine against the oracle: a fresh engine equals Make's
    image, then every output of the family's script in order: the batch's
    outputs, the whole state after it, the follow-up's outputs and the whole
    state again (every script takes an `image` after each call that can change
    the state). Returns the item count."""
    if KIND[name] == "cross":
        return run_cross(name, engine_cls, oracle_cls, check_state)
    G, P, L, st, b, _ = family(name)
    o = oracle_cls(G, P, L, st)
    with engine_cls(G, P, L) as e:
        check_state(e.store_state(), new_state(G, P, L), G, P, L, f"{name}: a fresh engine")
        e.load_state(st)
        got = SCRIPTS[KIND[name]](e, b)
        want = SCRIPTS[KIND[name]](o, b)
        compare_outputs(got, want, name, check_state, (G, P, L))
        check_state(e.store_state(), o.state(), G, P, L, name)
    return n_items(name)


def main():
    from oracle_lib import Oracle, assert_states_equal

    from multiraft_amd import Engine
    return run_all([(n,) for n in NAMES], lambda n: run_family(n, Engine, Oracle, assert_states_equal), n_items)


if __name__ == "__main__":
    sys.exit(main())
