"""Directed cases of the message-level AppendEntries handler by reference and
by value (mraft_handle_append_entries[_ex]: k_claim_ae, k_handle_set /
handle_one, defer_lanes, k_handle_deferred and its ordered fallback). Test
infrastructure only.

Every replica and every message is placed by hand (`World`): logs whose terms
depend strictly on the Index and on the row, dead slots poisoned with negative
words, ring heads off 0. A family is one script (`steps`) that runs unchanged
on three targets: the plain Python `Model` below, which restates
raft_append_entry.go:108-162 and the item rules of include/mraft.h from the
oracle's statement (gather-time copy of the entries, lowest item owns a slot,
the malformed classes, the Index domain, the capacity pre-check,
terms_sorted); the C oracle; and the engine. `run_script` returns, per call,
replies, item errors, the _ex records and an image of the whole state, and ends
with a follow-up batch on the same target (every second item of the last
batch, reversed: rows the first call claimed and source-marked are not in the
second, so stale epoch tags must read as nothing).

`geometry` is the only part that restates kernel rules, from the args array
alone: keys, runs, set heads and sizes (the k_claim_ae rule), the wave, lane
and stripe that serve an item, written / read (staged), the fallback's graph
(writers, reader counts, cycles) and the staged words per stripe. `cells`
names what a batch holds from `geometry` and the model's per-item record;
tests/test_handler_cases.py proves every claimed cell present."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from cases_program import run_all  # noqa: E402

from multiraft_amd._abi import (AE_ARGS, AE_ENTRIES_SORTED, AE_REPLY, AE_RESULT, FOLLOWER, ITEM_BAD_SLOT,  # noqa: E402
                                ITEM_DUP_SLOT, ITEM_LOG_FULL, LEADER, PERSIST_STATE)
from multiraft_amd.engine import copy_state, new_state  # noqa: E402

TOP = 2**31 - 2          # the Index domain's last Index
DEFAULT_STAGE = 1 << 22  # words (mraft_set_stage_capacity's default)
CYC_WALK = 32            # the fallback walks cycles of at most this many items
TM = 9000                # the term the messages carry unless a case says otherwise


# --------------------------------------------------------------------- builder
class World:
    """G x P replicas placed by hand. logs[slot] = (dummy, [terms of Index
    dummy, dummy + 1, ...])."""

    def __init__(self, G, P, L):
        self.G, self.P, self.L = G, P, L
        self.st = new_state(G, P, L)
        gp = G * P
        self.st["current_term"][:] = 1
        self.st["next_index"][:] = 1
        self.st["log_term"][:] = -(1 + np.arange(gp * L, dtype=np.int64)).astype(np.int32)  # poison, unique per word
        for s in range(gp):
            self.st["log_term"][s * L] = 0
        self.logs = {s: (0, [0]) for s in range(gp)}
        self.free = list(range(gp))

    def take(self, slot=None):
        slot = self.free[0] if slot is None else slot
        self.free.remove(slot)
        return slot

    def put(self, slot, terms, dummy=0, head=0, T=1, commit=None, voted=-1, role=FOLLOWER, nxt=None):
        L, st = self.L, self.st
        assert 1 <= len(terms) <= L and 0 <= head < L
        row = -(1 + slot * L + np.arange(L, dtype=np.int64)).astype(np.int32)
        for k, t in enumerate(terms):
            row[(head + k) % L] = t
        st["log_term"][slot * L:(slot + 1) * L] = row
        st["dummy_index"][slot], st["last_index"][slot] = dummy, dummy + len(terms) - 1
        st["log_head"][slot], st["current_term"][slot] = head, T
        st["commit_index"][slot] = st["last_applied"][slot] = dummy if commit is None else commit
        st["voted_for"][slot], st["state"][slot] = voted, role
        st["terms_sorted"][slot] = int(all(a <= b for a, b in zip(terms[1:], terms[2:])))
        st["next_index"][slot * self.P:(slot + 1) * self.P] = dummy + len(terms) if nxt is None else nxt
        self.logs[slot] = (dummy, list(terms))
        return slot

    def term(self, slot, idx):
        d, t = self.logs[slot]
        return t[idx - d] if 0 <= idx - d < len(t) else 0

    def entries(self, off, n):
        """The words a by-reference message names, as the gather-time copy reads them."""
        return read_entries(self.st, self.L, off, n)

    def msg(self, src, f, prev, n, term=TM, commit=0, flags=None, shift=0, leader_id=None, prev_term=None):
        a = np.zeros(1, dtype=AE_ARGS)[0]
        a["slot"], a["term"], a["prev_log_index"], a["n_entries"], a["leader_commit"] = f, term, prev, n, commit
        a["leader_id"] = src % self.P if leader_id is None else leader_id
        a["prev_log_term"] = self.term(src, prev) if prev_term is None else prev_term
        a["entries_offset"] = src * self.L + (prev + 1 - self.logs[src][0]) + shift
        if flags is None:  # the truthful claim, as the gather would make it from a sorted leader
            seq = [int(a["prev_log_term"])] + (self.entries(int(a["entries_offset"]), n) if n > 0 else [])
            flags = AE_ENTRIES_SORTED if all(x <= y for x, y in zip(seq, seq[1:])) else 0
        a["flags"] = flags
        return a


def read_entries(st, L, off, n):
    src, k0 = off // L, off % L
    h = int(st["log_head"][src])
    return [int(st["log_term"][src * L + (h + k0 + k) % L]) for k in range(n)]


def canon(tag, lo, hi):
    """Terms of Index lo..hi of the log `tag`: Index-dependent, rising."""
    return [tag * 1000 + i for i in range(lo, hi + 1)]


def batch(items):
    return np.array(items, dtype=AE_ARGS) if len(items) else np.zeros(0, dtype=AE_ARGS)


# ----------------------------------------------------------------------- model
def ref_ok(a, n_log, L):
    n, off = int(a["n_entries"]), int(a["entries_offset"])
    return not (n < 0 or off < 0 or off + n > n_log or off % L + n > L)


def index_ok(a):
    return int(a["prev_log_index"]) + int(a["n_entries"]) <= TOP


def ex_records(args, rep, err, P):
    """The _ex records as include/mraft.h states them, from args and replies."""
    res = np.zeros(len(args), dtype=AE_RESULT)
    for i, (a, r, e) in enumerate(zip(args, rep, err)):
        if e:
            res[i]["slot"] = res[i]["peer"] = -1
            continue
        f = int(a["slot"])
        res[i] = (f // P * P + int(a["leader_id"]), f % P, a["term"], a["prev_log_index"], a["n_entries"],
                  r["term"], r["success"], r["conflict_index"])
    return res


class Model:
    """mraft_handle_append_entries and mraft_gather_append_args in plain Python
    on a state image; `rec` keeps the last call's per-item record."""

    def __init__(self, G, P, L, st):
        self.G, self.P, self.L = G, P, L
        self.st = copy_state(st)
        self.rec = []

    def load_state(self, st):
        self.st = copy_state(st)

    def store_state(self):
        return copy_state(self.st)

    def _pos(self, s, idx):
        return s * self.L + (int(self.st["log_head"][s]) + idx - int(self.st["dummy_index"][s])) % self.L

    def _term(self, s, idx):
        return int(self.st["log_term"][self._pos(s, idx)])

    def gather_append_args(self, slots, peers):  # raft_append_entry.go:20-54
        st, P, L = self.st, self.P, self.L
        out, err = np.zeros(len(slots), dtype=AE_ARGS), np.zeros(len(slots), np.int32)
        for i, (s, p) in enumerate(zip(slots, peers)):
            s, p = int(s), int(p)
            assert 0 <= s < self.G * P and 0 <= p < P and p != s % P and st["state"][s] == LEADER
            prev = int(st["next_index"][s * P + p]) - 1
            d, last = int(st["dummy_index"][s]), int(st["last_index"][s])
            assert d <= prev <= last
            pt = self._term(s, prev)
            fl = st["terms_sorted"][s] and (prev > d or prev == last or pt <= self._term(s, prev + 1))
            out[i] = (s // P * P + p, st["current_term"][s], s % P, prev, pt, st["commit_index"][s], last - prev,
                      AE_ENTRIES_SORTED if fl else 0, s * L + prev + 1 - d)
        return out, err

    def handle(self, args, ents):
        st, P, L, gp = self.st, self.P, self.L, self.G * self.P
        n = len(args)
        rep, err = np.zeros(n, dtype=AE_REPLY), np.zeros(n, np.int32)
        rec = [dict(cls="none") for _ in range(n)]
        owner, copies = {}, [None] * n
        for i, a in enumerate(args):               # the lowest item addressed to a slot owns it
            s = int(a["slot"])
            if not 0 <= s < gp:
                err[i], rec[i]["cls"] = ITEM_BAD_SLOT, "badslot"
            elif s in owner:
                err[i], rec[i]["cls"] = ITEM_DUP_SLOT, "dup"
            else:
                owner[s] = i
        for i, a in enumerate(args):               # malformed classes; args.Entries copied at gather time (:50-54)
            if err[i]:
                continue
            k, off = int(a["n_entries"]), int(a["entries_offset"])
            if ents is None:
                good = ref_ok(a, gp * L, L) and index_ok(a)
            else:
                good = k >= 0 and off >= 0 and index_ok(a) and (k == 0 or off + k <= len(ents))
            if not good:
                err[i], rec[i]["cls"] = ITEM_BAD_SLOT, "bad"
            elif ents is None:
                copies[i] = read_entries(st, L, off, k) if k > 0 else []
            else:
                copies[i] = [int(x) for x in ents[off:off + k]] if k > 0 else []
        pristine = [list(c) if c is not None else None for c in copies]
        for i, a in enumerate(args):
            if not err[i]:
                err[i] = self._one(int(a["slot"]), a, pristine[i], rep[i], rec[i])
        self.rec = rec
        return rep, err, ex_records(args, rep, err, P)

    def _one(self, f, a, ent, r, R):               # HandleAppendEntries, raft_append_entry.go:108-162
        st, L = self.st, self.L
        T, prev, k = int(a["term"]), int(a["prev_log_index"]), int(a["n_entries"])
        d, last, cur = int(st["dummy_index"][f]), int(st["last_index"][f]), int(st["current_term"][f])
        matches = d <= prev <= last and self._term(f, prev) == int(a["prev_log_term"])
        first = next((j for j in range(k) if prev + 1 + j > last or self._term(f, prev + 1 + j) != ent[j]), None)
        if T >= cur and matches and first is not None and prev + k - d > L - 1:
            R["cls"] = "full"                      # the engine's capacity: rejected before any mutation
            return ITEM_LOG_FULL
        st["persist_dirty"][f] |= PERSIST_STATE    # defer rf.persist(), :111
        if T < cur:                                # :112-115
            r["term"], R["cls"] = cur, "stale"
            return 0
        if T > cur:                                # :116-118
            st["current_term"][f], st["voted_for"][f] = T, -1
            R["adopt"] = True
        st["state"][f] = FOLLOWER                  # :120
        if prev < d:                               # :123-127
            r["conflict_index"], R["cls"] = d + 1, "below"
            return 0
        if not matches:                            # :128-145
            r["term"] = T
            if prev > last:
                r["conflict_index"], R["cls"] = last + 1, "beyond"
            else:
                x, idx = self._term(f, prev), prev
                while idx > d + 1 and self._term(f, idx) == x:
                    idx -= 1
                r["conflict_index"] = idx
                R["cls"], R["scan"] = "mismatch", prev - idx
                R["scan_wraps"] = self._pos(f, idx) > self._pos(f, prev)
            return 0
        R["cls"] = "heartbeat" if k == 0 else "nowrite"
        if first is not None:                      # :149-155: truncate at the first mismatch, append the rest
            at = prev + 1 + first
            R["cls"] = "append" if at == last + 1 else "truncate"
            R["fol_wraps"] = self._pos(f, at) > self._pos(f, prev + k)
            for j in range(first, k):
                st["log_term"][self._pos(f, prev + 1 + j)] = ent[j]
            st["last_index"][f] = prev + k
            seq = [int(a["prev_log_term"])] + ent
            holds = bool(int(a["flags"]) & AE_ENTRIES_SORTED) and all(x <= y for x, y in zip(seq, seq[1:]))
            before = int(st["terms_sorted"][f])
            if not holds:
                st["terms_sorted"][f] = 0
                R["srt"] = "voided" if int(a["flags"]) & AE_ENTRIES_SORTED else "cleared"
            elif at == d + 1:
                st["terms_sorted"][f] = 1
                R["srt"] = "set"
            else:
                R["srt"] = "kept"
            R["srt_before"] = before
        if int(a["leader_commit"]) > int(st["commit_index"][f]):   # :157-160
            st["commit_index"][f] = min(int(a["leader_commit"]), int(st["last_index"][f]))
            R["commit"] = True
        r["term"], r["success"] = T, 1             # :161
        return 0


# -------------------------------------------------------------------- geometry
def stripe_of_wave(v, nb):
    """blockIdx & 7 of the workgroup that serves wave v of nb (the inverse of xcd_contiguous)."""
    per, rem = nb >> 3, nb & 7
    for x in range(8):
        lo = x * per + min(x, rem)
        if lo <= v < lo + per + (1 if x < rem else 0):
            return x
    raise AssertionError((v, nb))


def geometry(args, G, P, L, stage_cap=DEFAULT_STAGE):
    """What the engine's batching does with a by-reference batch, from the
    args alone (see the module docstring)."""
    n, gp = len(args), G * P
    n_log = gp * L
    ni = min(max(P - 1, 1), 7)
    key = []
    for a in args:
        s, off = int(a["slot"]), int(a["entries_offset"])
        if not 0 <= s < gp or not ref_ok(a, n_log, L) or not index_ok(a):
            key.append(None)
        else:
            key.append((off // L, off % L - (int(a["prev_log_index"]) + 1), int(a["prev_log_index"]) + int(a["n_entries"])))
    same = lambda i, j: 0 <= j < n and key[i] is not None and key[i] == key[j]  # noqa: E731
    pos, hd = [0] * n, [0] * n
    for i in range(n):
        while pos[i] < ni and same(i, i - pos[i] - 1):
            pos[i] += 1
        if key[i] is None or pos[i] >= ni:
            hd[i] = 1
        elif pos[i] == 0:
            hd[i] = 1
            while hd[i] < ni and same(i, i + hd[i]):
                hd[i] += 1
    head_of = [None] * n
    for i in range(n):
        for m in range(i, i + hd[i]):
            assert head_of[m] is None, "an item served twice"
            head_of[m] = i
    assert all(h is not None for h in head_of), "an item no set serves"
    nb = (n + ni - 1) // ni
    claimant, marked = {}, set()
    for i, a in enumerate(args):
        if 0 <= int(a["slot"]) < gp:
            claimant.setdefault(int(a["slot"]), i)
            if key[i] is not None and int(a["n_entries"]) > 0:
                marked.add(key[i][0])
    items = []
    for i, a in enumerate(args):
        s, k, off = int(a["slot"]), int(a["n_entries"]), int(a["entries_offset"])
        inr = 0 <= s < gp
        dup = inr and claimant[s] != i
        ok = ref_ok(a, n_log, L)
        written = inr and not dup and ok and s in marked
        srow = off // L if ok else None
        read = written and k > 0 and srow in claimant
        wraw = claimant[srow] if written and k > 0 and index_ok(a) and srow in claimant else -1
        writer = wraw if wraw >= 0 and ref_ok(args[wraw], n_log, L) else -1
        v = head_of[i] // ni
        items.append(dict(key=key[i], pos=pos[i], hd=hd[i], head=head_of[i], wave=v, lane=i - head_of[i],
                          head_lane=head_of[i] % ni, stripe=stripe_of_wave(v, nb), dup=dup, ok=ok, written=written,
                          read=read, wraw=wraw, writer=writer, kin=0, cyc=None, n=k))
    for it in items:
        if it["wraw"] >= 0:
            items[it["wraw"]]["kin"] += 1
    cycles = []
    for x, it in enumerate(items):
        if not it["written"] or it["cyc"] is not None:
            continue
        z, path = x, []
        while z >= 0 and z not in path and len(path) <= n:
            path.append(z)
            z = items[z]["writer"]
        if z == x:
            cyc = dict(members=path, least=min(path), len=len(path))
            cycles.append(cyc)
            for m in path:
                items[m]["cyc"] = cyc
    staged = [0] * 8
    for it in items:
        if it["read"]:
            staged[it["stripe"]] += it["n"]
    cap8 = stage_cap // 8
    return dict(items=items, ni=ni, nb=nb, staged=staged, cap8=cap8, fallback=max(staged) > cap8, cycles=cycles,
                nd=sum(it["written"] for it in items))


def path_of(geo, i):
    """How item i runs: main, or deferred in place / staged / chain (in place in
    the fallback) / cycbuf (from a cycle buffer; for a cycle longer than the
    walk whichever member the last workgroup meets first: 'cyclong')."""
    it = geo["items"][i]
    if not it["written"]:
        return "main"
    if not geo["fallback"]:
        return "staged" if it["read"] else "inplace"
    c = it["cyc"]
    if c is None:
        return "chain"
    if c["len"] > CYC_WALK:
        return "cyclong"
    return "cycbuf" if c["least"] == i else "chain"


# ----------------------------------------------------------------------- cells
def _run_lengths(geo):
    out, items, i = [], geo["items"], 0
    while i < len(items):
        j = i + 1
        while j < len(items) and items[i]["key"] is not None and items[j]["key"] == items[i]["key"]:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def cells(args, geo, rec, G, P, L, by_value=False, n_ents=0, cap=None):
    """The cells a batch holds, named from `geometry` and the model's record."""
    c, items, ni, n = set(), geo["items"] if geo else [], geo["ni"] if geo else 1, len(args)
    gp, cls = G * P, [r["cls"] for r in rec]
    if by_value:
        for a, r in zip(args, rec):
            c.add("V." + r["cls"])
            k, off = int(a["n_entries"]), int(a["entries_offset"])
            if k > 0 and off + k == n_ents and r["cls"] not in ("bad", "dup", "badslot"):
                c.add("V.exact_end")
            if k > 0 and off + k == n_ents + 1 and r["cls"] == "bad":
                c.add("V.one_over")
            if k == 0 and off > n_ents and r["cls"] == "heartbeat":
                c.add("V.hb_past")
        if n_ents == 0:
            c.add("V.empty_buffer")
        return c
    # K: runs, set heads, windows
    c.add(f"K.n{n}")
    c.add(f"K.waves{geo['nb']}")
    tagp = f"ni{ni}"
    for b, ln in _run_lengths(geo):
        if items[b]["key"] is None:
            continue
        c.add(f"K.run.{tagp}.len{ln}")
        if ln >= ni + 1 and 57 <= b <= 71 and b + ln > 64 + 7:
            c.add(f"K.edge.{b - 64:+d}")
        if b + ln == n and ln % ni != 0 and ln > 1:
            c.add("K.end_in_run")
        if ln > 1 and b // ni != (b + ln - 1) // ni:
            c.add("K.cross_window")
    for w in range(geo["nb"]):
        heads = [i for i in range(w * ni, min(n, (w + 1) * ni)) if items[i]["hd"]]
        if len(heads) == ni and ni > 1:
            c.add("K.window_all_heads")
    for i, it in enumerate(items):
        if it["hd"] >= 2:
            c.add(f"K.head_lane{it['head_lane']}")
    # near-miss keys beside a set: exactly one field of the key differs
    for i in range(n - 1):
        a, b = items[i]["key"], items[i + 1]["key"]
        if a and b and a != b and (items[i]["hd"] >= 2 or items[i + 1]["hd"] >= 2 or items[i]["pos"] > 0):
            diff = [f for f, x, y in zip(("row", "base", "end"), a, b) if x != y]
            if len(diff) == 1:
                c.add("K.near." + diff[0])
    # masked members and run splitters
    for i, it in enumerate(items):
        a = args[i]
        k, off, prev = int(a["n_entries"]), int(a["entries_offset"]), int(a["prev_log_index"])
        kind = None
        if cls[i] == "dup":
            w = items[[j for j in range(i) if int(args[j]["slot"]) == int(a["slot"])][0]]
            first = [j for j in range(i) if int(args[j]["slot"]) == int(a["slot"])][0]
            kind = "dup_of_malformed" if cls[first] == "bad" else "dup_same_wave" if w["wave"] == it["wave"] else "dup_other_wave"
        elif cls[i] == "badslot":
            kind = "slot_neg" if int(a["slot"]) < 0 else "slot_gp" if int(a["slot"]) == gp else None
        elif cls[i] == "bad":
            kind = ("n_neg" if k < 0 else "off_neg" if off < 0 else "idx_top" if not index_ok(a) else
                    "off_past" if off + k > gp * L else "row_over")
        elif it["written"]:
            kind = "deferred"
        elif cls[i] in ("stale", "below", "mismatch"):
            kind = cls[i]
        if kind is None:
            continue
        if it["key"] is not None:     # a member of a set, masked
            hd = items[it["head"]]["hd"]
            if hd >= 3:
                where = "head" if it["lane"] == 0 else "last" if it["lane"] == hd - 1 else "middle"
                c.add(f"K.mask.{kind}.{where}")
        else:                         # no key: it splits the run it stands in
            # (its run: the neighbours from the same sender, who carry the same prevLogTerm)
            mine = lambda j: 0 <= j < n and args[j]["prev_log_term"] == a["prev_log_term"]  # noqa: E731
            kp = items[i - 1]["key"] if mine(i - 1) else None
            kn = items[i + 1]["key"] if mine(i + 1) else None
            if kp is not None and kp == kn:
                c.add(f"K.mask.{kind}.middle")
            elif kn is not None and kp is None and i + 2 < n and items[i + 2]["key"] == kn:
                c.add(f"K.mask.{kind}.head")
            elif kp is not None and kn is None and i >= 2 and items[i - 2]["key"] == kp:
                c.add(f"K.mask.{kind}.last")
    merging = ("nowrite", "append", "truncate", "full", "heartbeat")
    for i, it in enumerate(items):
        if it["hd"] >= 3 and not any(items[m]["written"] for m in range(i, i + it["hd"])):
            ms = [m - i for m in range(i, i + it["hd"]) if cls[m] in merging]
            if not ms:
                c.add("K.nobody_merges")
            elif ms[0] == 0:
                c.add("K.first_merge.lane0")
            elif ms[0] == 1:
                c.add("K.first_merge.lane1")
            if ms and ms[0] == it["hd"] - 1 == ni - 1:
                c.add("K.first_merge.laneLast")
        if it["hd"] >= 2 and all(cls[m] == "heartbeat" for m in range(i, i + it["hd"])):
            c.add("K.hb_set")
        if (it["hd"] >= 2 and cls[i] == "heartbeat" and rec[i].get("src_q0") != int(args[i]["entries_offset"]) % L and
                any(cls[m] in ("append", "truncate") for m in range(i + 1, i + it["hd"]))):
            c.add("K.hb_heads_set")
        a = args[i]
        if int(a["n_entries"]) == 0:
            off = int(a["entries_offset"])
            if off % L == 0 and off > 0 and cls[i] == "heartbeat":
                c.add("K.hb_full.last" if off == gp * L else "K.hb_full.mid")
            if off == gp * L + 1 and cls[i] == "bad":
                c.add("K.hb_past.1")
            if off == gp * L + 5 * L and cls[i] == "bad":
                c.add("K.hb_past.5L")
        if int(a["prev_log_index"]) + int(a["n_entries"]) == TOP and cls[i] not in ("bad", "dup", "badslot"):
            c.add("K.idx_top_ok")
    # D: why an item is written; the staged item's claimant; class x path; rings; sizes
    for i, it in enumerate(items):
        a = args[i]
        s = int(a["slot"])
        if not 0 <= s < gp or it["dup"]:
            continue
        kinds = set()
        for j, b in enumerate(args):
            off = int(b["entries_offset"])
            if j == i or not 0 <= off < gp * L + 1 or off // L != s or not 0 <= int(b["slot"]) < gp:
                continue
            kinds.add("ref_bad" if not items[j]["ok"] else "idx_bad" if not index_ok(b) else
                      "heartbeat" if int(b["n_entries"]) == 0 else "dup" if items[j]["dup"] else "normal")
        if len(kinds) == 1 and it["ok"]:
            kd = kinds.pop()
            assert it["written"] == (kd in ("normal", "dup")), (i, kd)
            c.add(("D.written_by." if it["written"] else "D.not_written_by.") + kd)
        if it["read"]:
            w = claimant_of(args, gp, int(a["entries_offset"]) // L)
            c.add("D.staged_claimant." + ("ref_bad" if not items[w]["ok"] else "idx_bad" if not index_ok(args[w]) else "deferred"))
            off, k = int(a["entries_offset"]), int(a["n_entries"])
            c.add(f"D.staged_n{k}")
            if off // L == s and off % L != int(a["prev_log_index"]) + 1 - rec[i].get("dummy0", 0) and cls[i] in ("truncate", "append"):
                c.add("D.self_rewrite")
            q0 = rec[i].get("src_q0")
            if q0 is not None and q0 + k > L:
                w0 = L - q0
                c.add("D.src_wrap." + ("first" if w0 == 1 else "last" if w0 == k - 1 else "middle"))
            if rec[i].get("fol_wraps"):
                c.add("D.fol_wrap")
        if it["written"]:
            p = path_of(geo, i)
            names = [cls[i]]
            if cls[i] == "mismatch" and rec[i]["scan"] > 64 and rec[i]["scan_wraps"]:
                names.append("mismatch_scan65wrap")
            if rec[i].get("commit"):
                names.append("commit")
            if rec[i].get("adopt") and rec[i].get("voted0", -1) >= 0:
                names.append("adopt")
            if rec[i].get("srt") == "set" and rec[i].get("srt_before") == 0:
                names.append("sorted_holds")
            if rec[i].get("srt") == "voided" and rec[i].get("srt_before") == 1:
                names.append("sorted_voided")
            for nm in names:
                c.add(f"D.cls.{nm}.{p}")
    # S: the stage
    cap8, stg = geo["cap8"], geo["staged"]
    if any(stg):
        if cap is not None:
            c.add(f"S.cap{cap}")
        if max(stg) == cap8:
            c.add("S.exact_fill")
        if max(stg) == cap8 + 1:
            c.add("S.one_over")
        if sum(1 for x in stg if x) == 1 and max(stg) > cap8 and sum(stg) * 4 <= cap8 * 8:
            c.add("S.one_stripe_over_total_below")
        if all(stg):
            c.add("S.all_stripes")
        for i, it in enumerate(items):
            if it["hd"] >= 2:
                sz = [items[m]["n"] for m in range(i, i + it["hd"]) if items[m]["read"]]
                alone = stg[it["stripe"]] == sum(sz)
                if alone and len(sz) in (2, 3) and len(set(sz)) == len(sz) and sum(sz[:-1]) <= cap8 < sum(sz):
                    c.add(f"S.wave{len(sz)}_later_unfit")
    # F: the ordered fallback's graph (cells of the graph itself, whatever the stage)
    defer = [i for i, it in enumerate(items) if it["written"]]
    oncyc = {m for cy in geo["cycles"] for m in cy["members"]}
    for x in defer:
        it = items[x]
        if it["kin"] and x not in oncyc:
            c.add(f"F.readers{it['kin']}")
        if it["kin"] == 0 and x not in oncyc:
            z, ln = x, 0
            while z >= 0 and z not in oncyc:
                lastz, z, ln = z, items[z]["writer"], ln + 1
            if z < 0 and all(items[y]["kin"] <= 1 for y in _chain(items, x)):
                c.add(f"F.chain{ln}." + ("end_refbad" if items[lastz]["wraw"] >= 0 else "end_unwritten"))
            if z >= 0 and ln == 40 and items[z]["cyc"]["len"] == 3:
                c.add("F.chain40_into_cyc3")
    for cy in geo["cycles"]:
        fed = {m: items[m]["kin"] - 1 for m in cy["members"]}
        feeders = [x for x in defer if x not in oncyc and items[x]["writer"] in fed]
        tag = f"F.cyc{cy['len']}."
        if not any(fed.values()):
            c.add(tag + "alone")
        elif any(items[x]["kin"] >= 2 for x in feeders):
            c.add(tag + "tree2")
        elif max(fed.values()) >= 2:
            c.add(tag + "feed2")
        elif all(v == 1 for v in fed.values()):
            c.add(tag + ("feed_all" if cy["len"] > 1 else "feed_least"))
        elif sum(fed.values()) == 1:
            c.add(tag + ("feed_least" if fed[cy["least"]] else "feed_other"))
    if sum(1 for cy in geo["cycles"] if not any(items[m]["kin"] > 1 for m in cy["members"])) >= 2:
        c.add("F.two_cycles")
    return c


def _chain(items, x):
    out = []
    while x >= 0 and x not in out:
        out.append(x)
        x = items[x]["writer"]
    return out


def claimant_of(args, gp, slot):
    return next(j for j, b in enumerate(args) if int(b["slot"]) == slot)


# ---------------------------------------------------------------------- script
def followup(args):
    """Every second item of a batch, reversed, one term on."""
    b = args[::2][::-1].copy()
    b["term"] += 1
    return b


def steps_of(fam):
    """The family's script with its follow-up call appended."""
    st = list(fam["steps"])
    last = [s for s in st if s[0] == "call"]
    if last and fam.get("followup", True):
        st.append(("call", followup(last[-1][1]), last[-1][2]))
    return st


def run_script(target, fam, on_call=None):
    """The family's steps on a target (Model, Oracle or Engine, state loaded by
    the caller). Returns per call (args, replies, item errors, _ex records,
    state image)."""
    out, P = [], fam["P"]
    for step in steps_of(fam):
        if step[0] == "load":
            target.load_state(fam["st"])
            continue
        if step[0] == "gather":     # ("gather", slots, peers): the target's own gather, then the call
            args, gerr = target.gather_append_args(step[1], step[2])
            assert not np.asarray(gerr).any(), "a directed gather item failed"
            ents = None
        else:
            args, ents = step[1], step[2]
        if isinstance(target, Model):
            rep, err, res = target.handle(args, ents)
        else:
            try:
                rep, err, res = target.handle_append_entries(args, ents, results=True)
            except TypeError:       # the oracle: the records as the header states them
                rep, err = target.handle_append_entries(args, ents)
                res = ex_records(args, rep, err, P)
        out.append((np.array(args, copy=True), rep, err, res, target.store_state()))
        if on_call:
            on_call(len(out) - 1)
    return out


def compare_runs(got, want, G, P, L, check_state, ctx):
    assert len(got) == len(want), ctx
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), f"{ctx} call {k}: args differ"
        assert np.array_equal(g[2], w[2]), f"{ctx} call {k}: item errors differ at {np.nonzero(g[2] != w[2])[0][:8]}"
        assert np.array_equal(g[1], w[1]), f"{ctx} call {k}: replies differ at {np.nonzero(g[1] != w[1])[0][:8]}"
        assert np.array_equal(g[3], w[3]), f"{ctx} call {k}: _ex records differ at {np.nonzero(g[3] != w[3])[0][:8]}"
        check_state(g[4], w[4], G, P, L, f"{ctx} call {k}")


def annotate(fam, args, rec, st0):
    """What `cells` needs from the state before the call, added to the model's record."""
    L, gp = fam["L"], fam["G"] * fam["P"]
    for a, R in zip(args, rec):
        s, off = int(a["slot"]), int(a["entries_offset"])
        if 0 <= s < gp:
            R["dummy0"], R["voted0"] = int(st0["dummy_index"][s]), int(st0["voted_for"][s])
        if 0 <= off < gp * L:
            R["src_q0"] = (int(st0["log_head"][off // L]) + off % L) % L


# -------------------------------------------------------------------- families
def _fam(w, steps, claims, **kw):
    return dict(G=w.G, P=w.P, L=w.L, st=w.st, steps=steps, claims=set(claims), caps=kw.pop("caps", [None]), **kw)


def _leader(w, tag, d=5, last=40, head=None, T=TM):
    s = w.take()
    return w.put(s, canon(tag, d, last), dummy=d, head=(7 * tag) % w.L if head is None else head, T=T, role=LEADER,
                 commit=d)


def _fol(w, src, upto, d=None, tail=(), slot=None, **kw):
    """A follower whose log equals src's up to `upto`, then `tail`."""
    s = w.take(slot)
    d = w.logs[src][0] if d is None else d
    terms = [w.term(src, i) for i in range(d, upto + 1)] + list(tail)
    kw.setdefault("T", TM - 1 - s % 2)
    kw.setdefault("voted", s % w.P)
    kw.setdefault("head", (11 * s + 3) % w.L)
    return w.put(s, terms, dummy=d, **kw)


def fam_runs(P, L=64):
    """K: runs of same-key messages of length 1, ni - 1, ni, ni + 1, 2 ni, 2 ni + 1
    (ni = P - 1 = 1..7: mraft_create takes no P above 8, so the launcher's
    clamp of ni to 7 never acts)."""
    ni = min(P - 1, 7)
    lens = sorted({1, ni - 1, ni, ni + 1, 2 * ni, 2 * ni + 1} - {0})
    G = -(-(sum(lens) + len(lens) + 2) // P)
    w, items = World(G, P, L), []
    for t, ln in enumerate(lens):
        src = _leader(w, t + 1)
        for _ in range(ln):
            f = _fol(w, src, 12, tail=[70 + t, 71 + t])
            items.append(w.msg(src, f, 12, 3 + t % 3, commit=13))
    return _fam(w, [("load",), ("call", batch(items), None)], {f"K.run.ni{ni}.len{ln}" for ln in lens})


def _filler(w, src, k, items):
    """k single-message sets: the same source, a prev of their own each."""
    for j in range(k):
        f = _fol(w, src, 8 + j % 20)
        items.append(w.msg(src, f, 8 + j % 20, 2))


def fam_edge(L=61):
    """K: a run of 2 ni + 1 whose head stands at item 57..71 (P = 8), one call per position."""
    P, G = 8, 16
    w = World(G, P, L)
    src, rs = _leader(w, 1, last=45), _leader(w, 2, last=45)
    fill = [_fol(w, src, 8 + j % 20) for j in range(71)]
    run = [_fol(w, rs, 12, tail=[77]) for _ in range(15)]
    steps, claims = [], set()
    for off in range(-7, 8):
        items = [w.msg(src, f, 8 + j % 20, 2) for j, f in enumerate(fill[:64 + off])]
        items += [w.msg(rs, f, 12, 4, commit=14) for f in run]
        items += [w.msg(src, f, 8 + j % 20, 2) for j, f in enumerate(fill[64 + off:], 64 + off)][:3]
        steps += [("load",), ("call", batch(items), None)]
        claims.add(f"K.edge.{off:+d}")
    return _fam(w, steps, claims | {"K.cross_window"})


def fam_sizes(L=64):
    """K: batches of 1, 63, 64, 65 and 129 items, each ending inside a run (P = 5)."""
    P, G = 5, 28
    w = World(G, P, L)
    src, rs = _leader(w, 1), _leader(w, 2)
    fill = [_fol(w, src, 8 + j % 20) for j in range(127)]
    run = [_fol(w, rs, 12, tail=[77]) for _ in range(3)]
    steps, claims = [], set()
    for n in (1, 63, 64, 65, 129):
        k = min(2, n - 1)
        items = [w.msg(src, f, 8 + j % 20, 2) for j, f in enumerate(fill[:n - k - (1 if n > 1 else 0)])]
        items += [w.msg(rs, f, 12, 4) for f in run[:k + 1]]
        steps += [("load",), ("call", batch(items[:n] if n > 1 else items[-1:]), None)]
        claims.add(f"K.n{n}")
    return _fam(w, steps, claims | {"K.end_in_run"})


def fam_waves(L=64):
    """K: 1, 7, 8, 9, 15, 16, 17 and 25 waves (P = 3: two items per wave), every
    wave holding a set of two; and windows full of heads, a head on either lane."""
    P, G = 3, 36
    w = World(G, P, L)
    srcs = [_leader(w, t + 1) for t in range(25)]
    fols = [[_fol(w, s, 12, tail=[60 + t]) for _ in range(2)] for t, s in enumerate(srcs)]
    steps, claims = [], set()
    for nw in (1, 7, 8, 9, 15, 16, 17, 25):
        items = [w.msg(srcs[t], f, 12, 2 + t % 3, commit=13) for t in range(nw) for f in fols[t]]
        steps += [("load",), ("call", batch(items), None)]
        claims.add(f"K.waves{nw}")
    # shifted by one: the sets' heads on lane 1, every run crossing its window's end
    items = [w.msg(srcs[24], fols[24][0], 11, 2)] + [w.msg(srcs[t], f, 12, 2, commit=13) for t in range(6) for f in fols[t]]
    steps += [("load",), ("call", batch(items), None)]
    # a window of two heads
    items = [w.msg(srcs[t], fols[t][0], 12, 2) for t in range(4)]
    steps += [("load",), ("call", batch(items), None)]
    return _fam(w, steps, claims | {"K.head_lane0", "K.head_lane1", "K.cross_window", "K.window_all_heads"})


def fam_lanes(L=64):
    """K: a set's head on each lane 0..6 of its wave's window (P = 8), NI heads in one window."""
    P, G = 8, 12
    w = World(G, P, L)
    src, rs = _leader(w, 1), _leader(w, 2)
    fill = [_fol(w, src, 8 + j) for j in range(14)]
    run = [_fol(w, rs, 12, tail=[77]) for _ in range(3)]
    steps, claims = [], set()
    for q in range(7):
        items = [w.msg(src, f, 8 + j, 2) for j, f in enumerate(fill[:7 + q])] + [w.msg(rs, f, 12, 4) for f in run]
        steps += [("load",), ("call", batch(items), None)]
        claims.add(f"K.head_lane{q}")
    return _fam(w, steps, claims | {"K.window_all_heads", "K.cross_window"})


def fam_near(L=64):
    """K: beside a set of three, an item whose key differs in the row, the base
    or the end alone; the rows' contents differ, so a set cut without that
    field reads other entries."""
    P, G = 5, 8
    w = World(G, P, L)
    s1, s2 = _leader(w, 1), _leader(w, 2)
    items = []
    for field in ("row", "base", "end"):
        items += [w.msg(s1, _fol(w, s1, 12, tail=[77]), 12, 4, commit=14) for _ in range(3)]
        f = _fol(w, s1, 12, tail=[78])
        if field == "row":      # another leader's row with the same dummy: same base, same end
            items.append(w.msg(s2, f, 12, 4, prev_term=w.term(s1, 12)))
        elif field == "base":   # the same prev and count one ring position on
            items.append(w.msg(s1, f, 12, 4, shift=1))
        else:                   # one entry more from the same place
            items.append(w.msg(s1, f, 12, 5))
        items.append(w.msg(s2, _fol(w, s2, 9), 9, 1))   # a separator
    return _fam(w, [("load",), ("call", batch(items), None)], {"K.near.row", "K.near.base", "K.near.end"})


MASK_KINDS = ("dup_same_wave", "dup_other_wave", "dup_of_malformed", "n_neg", "off_neg", "off_past", "row_over",
              "idx_top", "slot_neg", "slot_gp", "deferred", "stale", "below", "mismatch")


def fam_masked(L=64):
    """K: a set of four (P = 5) with one member masked, at its head, in the
    middle and last, for every kind; the first merging member on lanes 0, 1
    and NI - 1; a set nobody merges in."""
    P, G = 5, 64
    w = World(G, P, L)
    gp = G * P
    s1 = _leader(w, 1)
    early = _fol(w, s1, 12, tail=[55])            # claimed in wave 0: the other waves' duplicates name it
    badf = _fol(w, s1, 12, tail=[56])
    items = [w.msg(s1, early, 10, 1), w.msg(s1, badf, 10, -1)]
    items += [w.msg(s1, _fol(w, s1, 9), 9, 1), w.msg(s1, _fol(w, s1, 8), 8, 1)]   # window 0 filled
    claims = set()
    tag = 2
    for kind in MASK_KINDS:
        for where, at in (("head", 0), ("middle", 2), ("last", 3)):
            src = _leader(w, tag)
            tag += 1
            while len(items) % 4:                  # each set in a window of its own
                items.append(w.msg(s1, _fol(w, s1, 7), 7, 1))
            fs = [_fol(w, src, 12, tail=[77]) for _ in range(4)]
            ms = [w.msg(src, f, 12, 4, commit=14) for f in fs]
            m = ms[at]
            if kind == "dup_same_wave":
                if at == 0:                        # the claimant stands before the set in the head's window
                    z = _fol(w, s1, 7)
                    items.append(w.msg(s1, z, 7, 1))
                    m["slot"] = z
                else:
                    m["slot"] = fs[0]
            elif kind == "dup_other_wave":
                m["slot"] = early
            elif kind == "dup_of_malformed":
                m["slot"] = badf
            elif kind == "n_neg":
                m["n_entries"] = -1
            elif kind == "off_neg":
                m["entries_offset"] = -1
            elif kind == "off_past":
                m["entries_offset"] = gp * L - 3
            elif kind == "row_over":
                m["entries_offset"] = src * L + L - 3
            elif kind == "idx_top":
                m["prev_log_index"] = TOP - 3
            elif kind == "slot_neg":
                m["slot"] = -1
            elif kind == "slot_gp":
                m["slot"] = gp
            elif kind == "deferred":               # its own row is another message's source
                ms.append(w.msg(fs[at], _fol(w, fs[at], 10), 10, 2))
            elif kind == "stale":
                w.st["current_term"][fs[at]] = TM + 1
            elif kind == "below":
                w.put(fs[at], canon(99, 14, 16), dummy=14, head=5, T=TM - 1)
            elif kind == "mismatch":
                w.put(fs[at], [w.term(src, 5), 33, 32, 31, 31, 31, 31, 31], dummy=5, head=60, T=TM - 1)
            claims.add(f"K.mask.{kind}.{where}")
            items += ms
    # the first merging member on lanes 0, 1 and NI - 1; nobody merging
    for lane in (0, 1, 3, None):
        src = _leader(w, tag)
        tag += 1
        while len(items) % 4:
            items.append(w.msg(s1, _fol(w, s1, 7), 7, 1))
        fs = [_fol(w, src, 12, tail=[77]) for _ in range(4)]
        for q, f in enumerate(fs):
            if lane is None or q < lane:
                w.st["current_term"][f] = TM + 1 + q
        items += [w.msg(src, f, 12, 4, commit=14) for f in fs]
    claims |= {"K.first_merge.lane0", "K.first_merge.lane1", "K.first_merge.laneLast", "K.nobody_merges"}
    # prev + n = 2^31 - 2 is inside the domain: answered (prev past last), not malformed
    f = _fol(w, s1, 9)
    items.append(w.msg(s1, f, TOP - 2, 2, prev_term=0, flags=0))
    items[-1]["entries_offset"] = s1 * L + 3
    return _fam(w, [("load",), ("call", batch(items), None)], claims | {"K.idx_top_ok"})


def fam_heartbeats(L=64):
    """K: a set of heartbeats; a full-log leader's heartbeats through the gather
    (entries_offset = (slot + 1) L) at a middle slot and at slot G P - 1; a
    heartbeat whose offset lies past the log image (malformed by reference,
    include/mraft.h)."""
    P, G = 3, 5
    w = World(G, P, L)
    gp = G * P
    s1 = w.put(w.take(0), canon(1, 5, 30), dummy=5, head=13, T=TM, role=LEADER, commit=20)
    f1, f2 = _fol(w, s1, 30, slot=1), _fol(w, s1, 30, slot=2)
    hb = [w.msg(s1, f1, 30, 0, commit=20), w.msg(s1, f2, 30, 0, commit=20)]
    # a heartbeat heading a set whose second member appends: the set's entries are read
    # through the heartbeat's source, so its ring head (13) counts
    lead = [w.msg(s1, _fol(w, s1, 30, slot=6), 30, 0, commit=20), w.msg(s1, _fol(w, s1, 28, slot=7), 28, 2, commit=20)]
    mid = w.put(w.take(4), canon(2, 3, 3 + L - 1), dummy=3, head=17, T=TM, role=LEADER, commit=30, nxt=3 + L)
    _fol(w, mid, 3 + L - 1, slot=3), _fol(w, mid, 3 + L - 1, slot=5)
    lastl = w.put(w.take(gp - 1), canon(3, 0, L - 1), dummy=0, head=L - 1, T=TM, role=LEADER, commit=9, nxt=L)
    _fol(w, lastl, L - 1, slot=gp - 3), _fol(w, lastl, L - 1, slot=gp - 2)
    past = []
    for extra in (1, 5 * L):
        m = w.msg(s1, _fol(w, s1, 30, slot=8 + (extra > 1)), 30, 0, commit=20)
        m["entries_offset"] = gp * L + extra
        past.append(m)
    steps = [("load",), ("call", batch(lead + past[:1] + hb + past[1:]), None), ("load",),
             ("gather", np.array([mid, mid, lastl, lastl], np.int32), np.array([0, 2, 0, 1], np.int32))]
    return _fam(w, steps, {"K.hb_set", "K.hb_heads_set", "K.hb_full.mid", "K.hb_full.last", "K.hb_past.1", "K.hb_past.5L"},
                followup=False)


V_CLASSES = ("stale", "below", "beyond", "mismatch", "nowrite", "append", "truncate", "full", "heartbeat", "dup",
             "badslot", "bad")


def fam_value(L=64):
    """V: entries in a caller's buffer (one message per wave): every reply
    class, a duplicate, a bad slot, a message ending on the buffer's last
    word and one word past it, a heartbeat whose offset lies past the buffer;
    then the same heartbeats with an empty buffer."""
    P, G = 3, 8
    w = World(G, P, L)
    src = _leader(w, 1, last=45)
    ents = np.array(canon(1, 13, 72), np.int32)      # Index 13.. of the leader's log, and on
    items = []

    def m(f, n, off=0, prev=12, **kw):
        a = w.msg(src, f, prev, n, **kw)
        a["entries_offset"] = off
        a["flags"] = AE_ENTRIES_SORTED
        return a
    st_f = _fol(w, src, 12)
    w.st["current_term"][st_f] = TM + 2
    items.append(m(st_f, 3))                                              # stale
    items.append(m(w.put(w.take(), canon(9, 20, 22), dummy=20, head=3, T=TM - 1), 3))   # below
    items.append(m(_fol(w, src, 9), 3))                                   # beyond
    items.append(m(w.put(w.take(), [w.term(src, 5)] + [44] * 7, dummy=5, head=62, T=TM), 3))  # mismatch
    items.append(m(_fol(w, src, 16), 3))                                  # nowrite
    items.append(m(_fol(w, src, 12), 3, commit=14))                       # append
    items.append(m(_fol(w, src, 13, tail=[71, 72]), 3))                   # truncate
    items.append(m(_fol(w, src, 12, d=5), L - 7))                         # 12 + 57 - 5 = L: full
    items.append(m(_fol(w, src, 12), 0))                                  # heartbeat
    dupf = _fol(w, src, 12)
    items += [m(dupf, 2), m(dupf, 3), m(w.G * w.P, 2), m(-1, 2)]          # duplicate, bad slots
    items.append(m(_fol(w, src, 12), 4, off=len(ents) - 4))               # ends on the buffer's last word
    items.append(m(_fol(w, src, 12), 4, off=len(ents) - 3))               # one word past it
    items.append(m(_fol(w, src, 12), 0, off=len(ents) + 9))               # a heartbeat's offset is never used
    hb = [m(_fol(w, src, 12), 0, off=0), m(_fol(w, src, 12), 0, off=5), m(_fol(w, src, 12), 1, off=0)]
    steps = [("load",), ("call", batch(items), ents), ("load",), ("call", batch(hb), np.zeros(0, np.int32))]
    return _fam(w, steps, {"V." + k for k in V_CLASSES} | {"V.exact_end", "V.one_over", "V.hb_past", "V.empty_buffer"},
                by_value=True, followup=False)


# ---- replicas that send and receive at once: the deferral families
D_CLASSES = ("stale", "below", "beyond", "mismatch", "nowrite", "truncate", "append", "full", "heartbeat", "commit",
             "adopt", "sorted_holds", "sorted_voided")


class Nodes:
    """Replicas with a common prefix (Index d..c of log 1) and suffixes of
    their own, each both a source row and a receiver."""

    def __init__(self, w, c=12, d=5):
        self.w, self.c, self.d, self.items, self.k = w, c, d, [], 0

    def node(self, kind="truncate", desc=False):
        w, c, d, L = self.w, self.c, self.d, self.w.L
        s = w.take()
        self.k += 1
        own = [2000 + 10 * s + j for j in range(6)]
        pre = canon(1, d, c)
        T, dd, terms, head = TM - 1 - s % 2, d, pre + own, (7 * s + 5) % L
        if desc:                                   # a sorted log of two entries; the word after it (dead here,
            terms = pre + own[:2]                  # shipped by a message of three) is one descent
        if kind == "stale":
            T = TM + 1
        elif kind == "below":
            dd, terms = c + 2, [3000 + s] + own
        elif kind == "beyond":
            terms = pre[:-2]
        elif kind == "append":
            terms = pre
        elif kind == "mismatch":
            terms = [pre[0], 77, 76] + [77] * (c - d - 2) + own   # the scan stops at the breaker, Index d + 2
            head = L - 4
        elif kind == "mismatch_long":              # a run of 80 equal terms, the ring's wrap inside it
            terms = pre[:15] + [76] + [77] * 80 + own
            head = L - 60
        elif kind == "full":
            dd, terms = d - 2, canon(1, d - 2, c) + own
        elif kind == "sorted_holds":               # the dummy at prev, an unsorted suffix: the proof is 0 before
            dd, terms = c, [pre[-1], own[0] + 3, own[0] + 1] + [own[0] + 10 + j for j in range(9)]
        w.put(s, terms, dummy=dd, head=head, T=T, voted=s % w.P, commit=dd)
        if desc:
            w.st["log_term"][s * L + (head + len(terms)) % L] = own[0] - 1
        return s

    def item(self, x, src, n=3, **kw):
        w, c = self.w, self.c
        prev = kw.pop("prev", c)
        kw.setdefault("prev_term", canon(1, prev, prev)[0])
        flags = kw.pop("flags", None)
        a = w.msg(src, x, prev, n, flags=0, **kw)
        # the words of the source row that stand prev + 1 - d past its dummy, whatever that dummy is
        a["entries_offset"] = src * w.L + (prev + 1 - self.d)
        if flags is None:
            seq = [int(a["prev_log_term"])] + (w.entries(int(a["entries_offset"]), n) if n > 0 else [])
            flags = AE_ENTRIES_SORTED if all(p <= q for p, q in zip(seq, seq[1:])) else 0
        a["flags"] = flags
        self.items.append(a)
        return len(self.items) - 1

    def match_source(self, x, src, n):
        """Make x's own suffix equal the entries it will receive (nothing to write)."""
        w = self.w
        d, t = w.logs[x]
        ent = w.entries(src * w.L + (self.c + 1 - self.d), n)
        keep = dict(dummy=d, head=int(w.st["log_head"][x]), T=int(w.st["current_term"][x]), voted=x % w.P, commit=d)
        w.put(x, t[:self.c - d + 1] + ent + [4000 + x], **keep)


def _d_kind(cl):
    return {"nowrite": "truncate", "heartbeat": "truncate", "commit": "truncate", "adopt": "truncate",
            "sorted_voided": "truncate"}.get(cl, cl)


def fam_dcls(L=61, long_scan=False):
    """D: a deferred item of every reply class, as a member of a 2-cycle (both
    staged; in the fallback the greater runs in place, the least from the cycle
    buffer) and deferred in place (its source row unclaimed), with main-launch
    neighbours. long_scan (L = 1,024): the mismatch's scan runs 80 entries
    with the follower's ring wrap inside it."""
    P, G = 5, 24
    w = World(G, P, L)
    c = 100 if long_scan else 12
    nd = Nodes(w, c=c)
    plain = nd.node("truncate")
    classes = ["mismatch_long"] if long_scan else list(D_CLASSES)
    claims = set()
    for cl in classes:
        kind = cl if cl == "mismatch_long" else _d_kind(cl)
        a, b, solo = (nd.node(kind, desc=cl == "sorted_voided") for _ in range(3))
        n = L - (c + 1 - nd.d) if cl == "full" else 3
        kw = dict(commit=c + 2) if cl == "commit" else {}
        if cl == "sorted_voided":
            kw["flags"] = AE_ENTRIES_SORTED
        if cl == "heartbeat":                      # reads nothing: deferred in place whatever its source
            nd.item(solo, plain, 0)
            nd.item(nd.node("append"), solo, 2)    # a main-launch reader of its row
            claims |= {"D.cls.heartbeat.inplace", "D.cls.heartbeat.chain"}
            continue
        if cl == "nowrite":
            # a's suffix equals b's entries and the reverse cannot both hold: a reads b, b reads a third row
            third = nd.node("truncate")
            nd.match_source(a, third, n)
            nd.match_source(b, a, n)
            nd.item(a, third, n), nd.item(b, a, n), nd.item(third, b, n)
            nd.match_source(solo, plain, n)
        else:
            nd.item(a, b, n, **kw), nd.item(b, a, n, **kw)
        nd.item(solo, nd.node(desc=True) if cl == "sorted_voided" else plain, n, **kw)
        nd.item(nd.node("append"), solo, 2)        # a main-launch reader of solo's row: solo is written, not read
        nm = "mismatch_scan65wrap" if long_scan else cl
        claims |= {f"D.cls.{nm}.{p}" for p in ("inplace", "staged", "chain", "cycbuf")}
    if long_scan:
        claims |= {f"D.cls.mismatch.{p}" for p in ("inplace", "staged", "chain", "cycbuf")}
    return _fam(w, [("load",), ("call", batch(nd.items), None)], claims, caps=[None, 0])


def fam_dwhy(L=64):
    """D: why an item is written (a normal reader, a rejected duplicate) and
    why not (only a heartbeat, an Index-malformed or a reference-malformed item
    names its row); a staged item whose source row's claimant is a deferred
    item, reference-malformed, or past the Index domain; a self-reference that
    rewrites the row it reads."""
    P, G = 5, 12
    w = World(G, P, L)
    nd = Nodes(w)
    plain = nd.node()
    A, B, C, D, E = (nd.node() for _ in range(5))
    for x in (A, B, C, D, E):
        nd.item(x, plain, 3)
    r1 = nd.node("append")
    nd.item(r1, A, 2)                                  # a normal reader of A
    nd.item(r1, B, 2)                                  # a rejected duplicate reads B
    i = nd.item(nd.node("append"), C, 2)
    nd.items[i]["prev_log_index"] = TOP - 1            # past the Index domain, its reference valid
    nd.item(nd.node("append"), D, 0)                   # a heartbeat names D
    i = nd.item(nd.node("append"), E, 2)
    nd.items[i]["n_entries"] = -2                      # reference-malformed
    # staged items and their claimants
    R1, R2, R3 = nd.node(), nd.node(), nd.node()
    X1, X2, X3 = nd.node(), nd.node(), nd.node()
    nd.item(R1, X1, 2)                                 # well-formed, deferred (X1 reads its row)
    i = nd.item(R2, plain, 2)
    nd.items[i]["n_entries"] = -1                      # reference-malformed: runs as bad in the main launch
    i = nd.item(R3, plain, 2)
    nd.items[i]["prev_log_index"] = TOP - 1            # past the Index domain: deferred, then bad
    for x, r in ((X1, R1), (X2, R2), (X3, R3)):
        nd.item(x, r, 4)
    for x in (X2, X3):
        nd.item(nd.node("append"), x, 2)               # main-launch readers make X2, X3 written
    S = nd.node()
    i = nd.item(S, S, 3)
    nd.items[i]["entries_offset"] += 2                 # its own row, two ring positions on
    claims = {"D.written_by.normal", "D.written_by.dup", "D.not_written_by.idx_bad", "D.not_written_by.heartbeat",
              "D.not_written_by.ref_bad", "D.staged_claimant.deferred", "D.staged_claimant.ref_bad",
              "D.staged_claimant.idx_bad", "D.self_rewrite"}
    return _fam(w, [("load",), ("call", batch(nd.items), None)], claims, caps=[None, 64, 0])


SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def fam_sizes_staged(L=1024):
    """D: staged copies of 1..513 words (two 256-word iterations and one word
    more), source rings whose staged range wraps at its first, a middle and its
    last word, receivers whose ring wraps under the append."""
    P, G = 5, 6
    w = World(G, P, L)
    nd = Nodes(w, c=12)
    for j, n in enumerate(SIZES):
        a, b = nd.node(), nd.node()
        # a's row: the staged range [q0, q0 + n) wraps after its first word, in the middle, before its last
        q_rel = 12 + 1 - nd.d
        want = {0: 1, 1: max(1, n // 2), 2: n - 1}[j % 3]
        if n >= 2:
            d, t = w.logs[a]
            w.put(a, t, dummy=d, head=(L - want - q_rel) % L, T=TM - 1, voted=a % P, commit=d)
        d, t = w.logs[b]
        w.put(b, t, dummy=d, head=(L - 12 + d - 2) % L, T=TM - 2, voted=b % P, commit=d)   # the receiver's append wraps
        nd.item(b, a, n), nd.item(a, b, n)
    claims = {f"D.staged_n{n}" for n in SIZES} | {"D.src_wrap.first", "D.src_wrap.middle", "D.src_wrap.last", "D.fol_wrap"}
    return _fam(w, [("load",), ("call", batch(nd.items), None)], claims, caps=[None, 0])


def _pairs(w, nd, sizes):
    """2-cycles at P = 2 (one item per wave): pair j's items stand at 2 j and 2 j + 1."""
    for na, nb in sizes:
        a, b = nd.node(), nd.node()
        nd.item(a, b, na), nd.item(b, a, nb)


def fam_stage(over):
    """S: sixteen waves, two per stripe, a 2-cycle in each stripe. Stripe 0
    stages 5 + 3 = 8 words, the others 1 + 1: with 71 words of stage (8 per
    stripe) stripe 0 is filled exactly. `over`: 5 + 4 instead."""
    P, G, L = 2, 8, 64
    w = World(G, P, L)
    nd = Nodes(w)
    _pairs(w, nd, [(5, 4 if over else 3)] + [(1, 1)] * 7)
    claims = {"S.all_stripes", "S.one_over" if over else "S.exact_fill"} | {f"S.cap{c}" for c in (0, 7, 8, 71)}
    return _fam(w, [("load",), ("call", batch(nd.items), None)], claims, caps=[71, 0, 7, 8, None])


def fam_stage_one_stripe():
    """S: nine staged words, all in stripe 3, with 1,024 words of stage (128 per
    stripe... the batch stages) and with 71 (8 per stripe: the fallback, the
    total far below the capacity)."""
    P, G, L = 2, 10, 64
    w = World(G, P, L)
    nd = Nodes(w)
    src = _leader(w, 7)
    for j in range(6):                          # waves 0..5 (stripes 0..2): plain messages
        nd.items.append(w.msg(src, _fol(w, src, 12), 12, 2))
    _pairs(w, nd, [(5, 4)])                     # waves 6, 7 of 16: stripe 3
    for j in range(8):
        nd.items.append(w.msg(src, _fol(w, src, 12), 12, 2))
    return _fam(w, [("load",), ("call", batch(nd.items), None)], {"S.one_stripe_over_total_below"}, caps=[71, 1024])


def fam_stage_wave(k):
    """S: k staged members of different sizes in one set (P = 5), alone in their
    stripe: the earlier fit the stripe, the last does not."""
    P, G, L = 5, 8, 64
    w = World(G, P, L)
    nd = Nodes(w)
    R = nd.node()
    ms = [nd.node() for _ in range(k)]
    for j, x in enumerate(ms):                 # one key: prev one lower, one entry more
        nd.item(x, R, 3 + j, prev=12 - j)
    for x in ms:
        nd.item(nd.node("append"), x, 2)       # their rows are read: written
    nd.item(R, ms[0], 2)                        # R is claimed: the members are read too
    cap = 8 * (sum(3 + j for j in range(k)) - 1)
    return _fam(w, [("load",), ("call", batch(nd.items), None)], {f"S.wave{k}_later_unfit"}, caps=[cap, None])


CYC_LENS = (1, 2, 3, 31, 32, 33, 40)
CYC_VARIANTS = ("alone", "feed_least", "feed_other", "feed_all", "feed2", "tree2")


def cyc_variants(ln):
    """A cycle of one has no other member, and feeding all of it is feeding its least."""
    return [v for v in CYC_VARIANTS if not (ln == 1 and v in ("feed_other", "feed_all"))]


KINDS_ROT = ("truncate", "append", "stale", "truncate", "beyond", "mismatch", "below")


def _cycle(nd, ln, variant, k0):
    """A cycle of ln nodes whose least item is not its first-made node, with feeders by variant."""
    xs = [nd.node(KINDS_ROT[(k0 + j) % len(KINDS_ROT)]) for j in range(ln)]
    order = xs[1:] + xs[:1]                    # items in this order: the least item sits at xs[1]
    for j, x in enumerate(order):
        i = nd.item(x, xs[(xs.index(x) + 1) % ln], 2 + j % 3)
        if ln == 1:
            nd.items[i]["entries_offset"] += 2     # its own row, two ring positions on
    least, other = order[0], order[len(order) // 2]

    def feeder(at, leaf=True):
        f = nd.node()
        nd.item(f, at, 2)
        if leaf:
            nd.item(nd.node("append"), f, 1)       # a main-launch reader: the feeder is written, so deferred
        return f
    if variant == "feed_least":
        feeder(least)
    elif variant == "feed_other":
        feeder(other)
    elif variant == "feed_all":
        for x in xs:
            feeder(x)
    elif variant == "feed2":
        feeder(other), feeder(other)
    elif variant == "tree2":
        f = feeder(other, leaf=False)
        feeder(f), feeder(f)


def fam_cycles(ln, L=64):
    """F: cycles of ln items in every variant, as disjoint components of one batch."""
    P = 8
    variants = cyc_variants(ln)
    need = sum(ln + {"alone": 0, "feed_least": 2, "feed_other": 2, "feed_all": 2 * ln, "feed2": 4, "tree2": 5}[v]
               for v in variants) + 2
    w = World(-(-(need + 1) // P), P, L)
    nd = Nodes(w)
    for k, v in enumerate(variants):
        _cycle(nd, ln, v, k)
    if ln == 2:
        _cycle(nd, 2, "alone", 5)                  # a second cycle nothing feeds
    claims = {f"F.cyc{ln}.{v}" for v in variants} | ({"F.two_cycles"} if ln == 2 else set())
    return _fam(w, [("load",), ("call", batch(nd.items), None)], claims, caps=[0, None], grids=True)


def fam_chains(L=64):
    """F: chains of 1, 2, 3 and 40 items ending at an item nobody writes and at
    a reference-malformed claimant; a writer with 1, 2, 3 and 70 readers; a
    40-chain into a 3-cycle."""
    P, G = 8, 40
    w = World(G, P, L)
    nd = Nodes(w)
    plain = nd.node()
    claims = set()

    def chain(ln, end, k0):
        xs = [nd.node(KINDS_ROT[(k0 + j) % len(KINDS_ROT)]) for j in range(ln)]
        for j, x in enumerate(xs[:-1]):
            nd.item(x, xs[j + 1], 2 + j % 3)
        return xs
    for ln in (1, 2, 3, 40):
        for end in ("end_unwritten", "end_refbad"):
            xs = chain(ln, end, ln)
            if end == "end_unwritten":
                nd.item(xs[-1], plain, 2)              # its source row has no claimant
            else:
                bad = nd.node()
                i = nd.item(bad, plain, 2)
                nd.items[i]["n_entries"] = -3
                nd.item(xs[-1], bad, 2)
            nd.item(nd.node("append"), xs[0], 2)       # a main-launch reader: the chain's first item is written
            claims.add(f"F.chain{ln}.{end}")
    for k in (1, 2, 3, 70):
        wr = nd.node()
        nd.item(wr, plain, 3)
        for _ in range(k):
            r = nd.node()
            nd.item(r, wr, 2)
            nd.item(nd.node("append"), r, 1)           # the reader itself written: deferred, counted at wr
        claims.add(f"F.readers{k}")
    xs = chain(40, None, 3)
    cyc = [nd.node() for _ in range(3)]
    for j, x in enumerate(cyc):
        nd.item(x, cyc[(j + 1) % 3], 2)
    nd.item(xs[-1], cyc[1], 2)
    nd.item(nd.node("append"), xs[0], 2)
    claims.add("F.chain40_into_cyc3")
    return _fam(w, [("load",), ("call", batch(nd.items), None)], claims, caps=[0, None], grids=True)


def fam_small_batches(L=64):
    """F: batches of 1..9 items at stage 0 (the deferred grid is min(n, grid)):
    a self-reference, then 2-cycles and a chain, one call per size."""
    P, G = 5, 4
    w = World(G, P, L)
    nd = Nodes(w)
    xs = [nd.node() for _ in range(9)]
    steps = []
    for n in range(1, 10):
        nd.items = []
        i = nd.item(xs[0], xs[0], 2)
        nd.items[i]["entries_offset"] += 2
        for j in range(1, n):
            nd.item(xs[j], xs[j % (n - 1) + 1] if n > 2 else xs[0], 2)
        steps += [("load",), ("call", batch(nd.items), None)]
    return _fam(w, steps, {f"K.n{n}" for n in range(1, 10)}, caps=[0], grids=True)


GRID_MINS = (None, 1, 3, 8, 9)      # MRAFT_DEFER_GRID_MIN for the families marked `grids`

FAMILIES = ([(f"runs_P{P}", fam_runs, (P,)) for P in (2, 3, 4, 5, 6, 7, 8)] +
            [("runs_P5_L61", fam_runs, (5, 61)), ("edge", fam_edge, ()), ("sizes", fam_sizes, ()),
             ("waves", fam_waves, ()), ("lanes", fam_lanes, ()), ("near", fam_near, ()), ("masked", fam_masked, ()),
             ("heartbeats", fam_heartbeats, ()), ("value", fam_value, ()),
             ("dcls", fam_dcls, ()), ("dcls_scan", fam_dcls, (1024, True)), ("dwhy", fam_dwhy, ()),
             ("staged_sizes", fam_sizes_staged, ()),
             ("stage_exact", fam_stage, (False,)), ("stage_over", fam_stage, (True,)),
             ("stage_one_stripe", fam_stage_one_stripe, ()), ("stage_wave2", fam_stage_wave, (2,)),
             ("stage_wave3", fam_stage_wave, (3,))] +
            [(f"cyc{ln}", fam_cycles, (ln,)) for ln in CYC_LENS] +
            [("chains", fam_chains, ()), ("small_batches", fam_small_batches, ())])
NAMES = [n for n, _, _ in FAMILIES]
# by reference, with more than one call or a deferral: also run as device-resident calls back to back
DEVICE_FAMILIES = ("masked", "dwhy", "dcls", "chains")
_cache = {}


def family(name):
    """A family, built once; callers must not modify it."""
    if name not in _cache:
        fn, a = next((f, a) for n, f, a in FAMILIES if n == name)
        _cache[name] = fn(*a)
    return _cache[name]


def modes(name):
    """The (stage capacity, MRAFT_DEFER_GRID_MIN) pairs a family runs under on an engine."""
    fam = family(name)
    out = [(cap, None) for cap in fam["caps"]]
    if fam.get("grids"):
        out += [(0, g) for g in GRID_MINS[1:]]
    return out


_want = {}


def oracle_run(name, oracle_cls):
    """The oracle's answers of a family (computed once, shared, never modified)."""
    if name not in _want:
        fam = family(name)
        _want[name] = run_script(oracle_cls(fam["G"], fam["P"], fam["L"], fam["st"]), fam)
    return _want[name]


def run_family(name, engine_cls, oracle_cls, check_state, cap=None, gmin=None):
    """The family on an engine against the oracle under one mode. Returns the number of calls."""
    fam = family(name)
    G, P, L = fam["G"], fam["P"], fam["L"]
    want = oracle_run(name, oracle_cls)
    old = os.environ.get("MRAFT_DEFER_GRID_MIN")
    if gmin is not None:
        os.environ["MRAFT_DEFER_GRID_MIN"] = str(gmin)   # read at mraft_create
    try:
        with engine_cls(G, P, L) as e:
            if cap is not None:
                e.set_stage_capacity(cap)
            e.load_state(fam["st"])
            got = run_script(e, fam)
    finally:
        if gmin is not None:
            os.environ.pop("MRAFT_DEFER_GRID_MIN")
            if old is not None:
                os.environ["MRAFT_DEFER_GRID_MIN"] = old
    compare_runs(got, want, G, P, L, check_state, f"{name} stage {cap} grid {gmin}")
    return len(got)


def main():
    """Every family under every mode on the library MRAFT_LIB names, then the
    bounds-checking build's counters when it has them: one JSON line."""
    import ctypes

    from oracle_lib import Oracle, assert_states_equal

    from multiraft_amd import Engine, _abi

    def violations():
        viol = {}
        for fn in ("mraft_debug_bounds_kernels", "mraft_debug_bounds_deferred", "mraft_debug_bounds_tick"):
            f = getattr(_abi.lib(), fn, None)
            if f is not None:
                f.restype, f.argtypes = ctypes.c_longlong, [ctypes.c_int]
                viol[fn] = int(f(0))
        return {"violations": viol}

    return run_all([(n, cap, gmin) for n in NAMES for cap, gmin in modes(n)],
                   lambda n, cap, gmin: run_family(n, Engine, Oracle, assert_states_equal, cap, gmin),
                   lambda *run: 0, violations)


if __name__ == "__main__":
    sys.exit(main())
