"""Model of the co-resident calls under a reachability mask
(mraft_set_reachable, include/mraft.h): the tick, the election round and the
clock step, composed from the CPU oracle's message-level calls in the fused
calls' own order. The oracle has no mask and gets none: a message that the mask
drops is simply not handed to the oracle's handler, and its reply is not folded.
Test infrastructure only.

  masked_tick     gather (a3) for every follower -> handle for the delivered
                  ones -> one process_*_replies call per peer rank, ascending
                  (Go evaluates a1 after every reply, so folding AE and IS
                  replies peer by peer is exact) -> the MRAFT_G_* word rebuilt
                  from those calls' outputs.
  masked_round    timers_model.deliver_round restated with the delivery filter,
                  then timers_model.tally_round as it is.
  ReachModel      TimersModel with a mask: clock_step on top of the two, rule E
                  restricted to the replicas that heard the sender.
"""
from __future__ import annotations

import numpy as np

from multiraft_amd import _abi
from multiraft_amd._abi import AE_RESULT, IS_RESULT, LEADER, RV_ARGS, RV_RESULT
from timers_model import TimersModel, tally_round

ITEM_PREV_BEYOND_LAST, ITEM_NEED_SNAPSHOT = 1, 4


def full_mask(G, P):
    return np.full(G, (1 << P) - 1, np.uint8)


def connected(reach, G, P):
    """bool[G, P]: bit p of reach[g]."""
    return ((np.asarray(reach, np.int64)[:, None] >> np.arange(P)[None, :]) & 1).astype(bool)


def masked_tick(o, lp, reach, record=None):
    """One tick of every group on the oracle `o` under `reach` (uint8[G]).
    Returns the group flags. `record` (a dict) receives, per group, what the
    presence tests count: the delivery class of every follower."""
    G, P = o.G, o.P
    st = o.st
    lp = np.asarray(lp, np.int32)
    conn = connected(reach, G, P)
    gf = np.zeros(G, np.int32)
    gf[lp >= P] = _abi.G_ERROR
    inr = (lp >= 0) & (lp < P)
    ld = np.arange(G, dtype=np.int64) * P + np.where(inr, lp, 0)
    isl = inr & (st["state"][ld] == LEADER)
    bad = isl & (st["commit_index"][ld] < st["dummy_index"][ld])
    gf[bad] = _abi.G_ERROR
    run = isl & ~bad
    if record is not None:
        record.update(run=run.copy(), delivered=np.zeros((G, P), bool), ae=np.zeros((G, P), bool),
                      snap=np.zeros((G, P), bool), reply_success=np.zeros((G, P), bool),
                      reply_term_higher=np.zeros((G, P), bool), log_full=np.zeros((G, P), bool),
                      n_entries=np.zeros((G, P), np.int64))
    if P < 2 or not run.any():
        gf[run] = _abi.G_ACTIVE
        return gf
    # 1. a3 for every follower of every running group (the leader's own step)
    gs = np.nonzero(run)[0]
    peers = np.arange(P)[None, :].repeat(len(gs), 0)
    fol = peers != lp[gs][:, None]
    sl = np.repeat(ld[gs], P - 1).astype(np.int32)
    pr = peers[fol].astype(np.int32)
    grp = np.repeat(gs, P - 1)
    args, aerr = o.gather_append_args(sl, pr)
    assert np.isin(aerr, (0, ITEM_PREV_BEYOND_LAST, ITEM_NEED_SNAPSHOT)).all()
    panic = np.zeros(G, bool)
    panic[grp[aerr == ITEM_PREV_BEYOND_LAST]] = True
    need = np.zeros(G, bool)
    need[grp[aerr == ITEM_NEED_SNAPSHOT]] = True
    gf[run] = _abi.G_ACTIVE
    gf[need & run] |= _abi.G_NEED_SNAPSHOT
    gf[panic] = _abi.G_ERROR | np.where(need[panic], _abi.G_NEED_SNAPSHOT, 0)
    # 2. the deliveries: leader and follower both connected
    dl = conn[grp, lp[grp]] & conn[grp, pr] & ~panic[grp]
    is_snap = aerr == ITEM_NEED_SNAPSHOT
    commit0 = st["commit_index"][ld].copy()
    ae_i = np.nonzero(dl & ~is_snap)[0]
    is_i = np.nonzero(dl & is_snap)[0]
    ae_items = np.zeros(0, AE_RESULT)
    ae_peer = np.zeros(0, np.int64)
    if len(ae_i):
        a = args[ae_i].copy()
        fslot = grp[ae_i] * P + pr[ae_i]
        assert np.array_equal(a["slot"], fslot)
        fc = a["leader_commit"] > st["commit_index"][fslot]
        rep, herr = o.handle_append_entries(a, None)
        assert np.isin(herr, (0, _abi.ITEM_LOG_FULL)).all()
        np.bitwise_or.at(gf, grp[ae_i][herr != 0], _abi.G_LOG_FULL)
        np.bitwise_or.at(gf, grp[ae_i][(herr == 0) & (rep["success"] != 0) & fc], _abi.G_FOLLOWER_COMMIT)
        okk = herr == 0
        ae_items = np.zeros(int(okk.sum()), AE_RESULT)
        ae_items["slot"] = sl[ae_i][okk]
        ae_items["peer"] = pr[ae_i][okk]
        ae_items["args_term"] = a["term"][okk]
        ae_items["args_prev_log_index"] = a["prev_log_index"][okk]
        ae_items["args_n_entries"] = a["n_entries"][okk]
        ae_items["reply_term"] = rep["term"][okk]
        ae_items["reply_success"] = rep["success"][okk]
        ae_items["reply_conflict_index"] = rep["conflict_index"][okk]
        ae_peer = pr[ae_i][okk].astype(np.int64)
        if record is not None:
            record["ae"][grp[ae_i], pr[ae_i]] = True
            record["n_entries"][grp[ae_i], pr[ae_i]] = a["n_entries"]
            record["log_full"][grp[ae_i], pr[ae_i]] = herr != 0
            record["reply_success"][grp[ae_i][okk], pr[ae_i][okk]] = rep["success"][okk] != 0
            record["reply_term_higher"][grp[ae_i][okk], pr[ae_i][okk]] = rep["term"][okk] > a["term"][okk]
    is_items = np.zeros(0, IS_RESULT)
    is_peer = np.zeros(0, np.int64)
    if len(is_i):
        ia, ierr = o.gather_install_snapshot_args(sl[is_i], pr[is_i])
        assert not ierr.any() and np.array_equal(ia["slot"], grp[is_i] * P + pr[is_i])
        rep, fl, herr = o.handle_install_snapshot(ia)
        np.bitwise_or.at(gf, grp[is_i][herr != 0], _abi.G_FOLLOWER_PANIC)
        np.bitwise_or.at(gf, grp[is_i][(herr == 0) & ((fl & _abi.F_SNAPSHOT_INSTALLED) != 0)],
                         _abi.G_SNAPSHOT_INSTALLED)
        okk = herr == 0
        is_items = np.zeros(int(okk.sum()), IS_RESULT)
        is_items["slot"] = sl[is_i][okk]
        is_items["peer"] = pr[is_i][okk]
        is_items["args_term"] = ia["term"][okk]
        is_items["args_last_included_index"] = ia["last_included_index"][okk]
        is_items["reply_term"] = rep["term"][okk]
        is_peer = pr[is_i][okk].astype(np.int64)
        if record is not None:
            record["snap"][grp[is_i], pr[is_i]] = True
            record["reply_term_higher"][grp[is_i][okk], pr[is_i][okk]] = rep["term"][okk] > ia["term"][okk]
    if record is not None:
        record["delivered"][grp[dl], pr[dl]] = True
    # 3. the fold: the replies that exist, one peer rank per call (one reply per
    # leader and call, so every segment is one item)
    for p in range(P):
        for items, peer, fold in ((ae_items, ae_peer, o.process_append_replies),
                                  (is_items, is_peer, o.process_install_snapshot_replies)):
            it = items[peer == p]
            if not len(it):
                continue
            fl, ferr = fold(it)
            assert not ferr.any()
            np.bitwise_or.at(gf, it["slot"][(fl & _abi.F_STEPPED_DOWN) != 0] // P, _abi.G_STEPPED_DOWN)
    # 4. the leader's commit
    moved = run & ~panic & (st["commit_index"][ld] != commit0)
    gf[moved] |= _abi.G_COMMITTED
    return gf


def masked_deliver_round(node, G, P, cslots, reach):
    """timers_model.deliver_round with the delivery filter: candidate c's
    RequestVote reaches voter v iff both bits of reach[g] are set. Returns
    (items, seg, granted); a candidate with no reply has no segment."""
    granted = np.zeros(G * P, bool)
    if not len(cslots):
        return None, None, granted
    args, err = node.start_election(cslots)              # local: connected or not
    assert not err.any()
    if P < 2:
        return None, None, granted
    conn = connected(reach, G, P).reshape(-1)
    grp = cslots // P
    rank = np.arange(len(cslots)) - np.searchsorted(grp, grp)
    res = np.zeros((len(cslots), P), dtype=RV_RESULT)
    got = np.zeros((len(cslots), P), bool)
    for k in range(int(rank.max()) + 1):
        idx = np.nonzero(rank == k)[0]
        c = cslots[idx].astype(np.int64)
        voters = (c // P)[:, None] * P + np.arange(P)[None, :]
        keep = (voters != c[:, None]) & conn[voters] & conn[c][:, None]
        if not keep.any():
            continue
        vs = voters[keep]
        src = np.repeat(idx, P).reshape(len(idx), P)[keep]
        a = np.zeros(len(vs), dtype=RV_ARGS)
        a["slot"] = vs
        a["candidate_id"] = cslots[src] % P
        for f in ("term", "last_log_index", "last_log_term"):
            a[f] = args[f][src]
        rep, herr = node.handle_request_vote(a)
        assert not herr.any()
        granted[vs[rep["vote_granted"] != 0]] = True
        r = np.zeros(len(vs), dtype=RV_RESULT)
        r["slot"], r["peer"] = cslots[src], vs % P
        r["args_term"], r["reply_term"], r["vote_granted"] = a["term"], rep["term"], rep["vote_granted"]
        res[src, vs % P] = r
        got[src, vs % P] = True
    if not got.any():
        return None, None, granted
    items = res[got]                                     # voter order within each candidate
    n = got.sum(axis=1)
    seg = np.concatenate(([0], np.cumsum(n[n > 0]))).astype(np.int64)
    return items, seg, granted


def masked_round(node, G, P, cslots, reach):
    """One election round under the mask: (group flags, granted, became)."""
    items, seg, granted = masked_deliver_round(node, G, P, np.asarray(cslots, np.int32), reach)
    gf, became, _ = tally_round(node, G, P, items, seg)
    return gf, granted, became


def masked_election_rounds(o, cand_mask, reach):
    """mraft_election_rounds under the mask on the oracle `o`: per round the
    replicas of cand_mask[r] that are not Leader time out."""
    G, P = o.G, o.P
    gf = np.zeros(G, np.int32)
    for m in np.asarray(cand_mask, np.uint8):
        cand = connected(m, G, P).reshape(-1) & (o.st["state"] != LEADER)
        f, _, _ = masked_round(o, G, P, np.nonzero(cand)[0].astype(np.int32), reach)
        gf |= f
    return gf


class ReachModel(TimersModel):
    """TimersModel whose co-resident calls honour `reach` (None: no mask; the
    model then is TimersModel itself)."""

    def __init__(self, G, P, L, st=None):
        super().__init__(G, P, L, st)
        self.reach = None
        self.tick_record = None

    def set_reachable(self, reach):
        self.reach = None if reach is None else np.array(reach, np.uint8)

    def clock_step(self, now, send_all=False):
        if self.reach is None:
            return super().clock_step(now, send_all)
        G, P, o = self.G, self.P, self.o
        hb = self.cfg[1]
        slots = self._slots()
        dl = self._edl(slots, now)
        role0 = o.st["state"].copy()
        # A: local
        edue, hdue = self.ed <= now, self.hd <= now
        self.ed[edue] = dl[edue]
        cand = edue & (role0 != LEADER)
        fired = hdue & (role0 == LEADER)
        self.hd[hdue & (role0 != LEADER)] = now + hb
        bits = (cand.reshape(G, P).astype(np.int64) << np.arange(P)).sum(axis=1).astype(np.uint8)
        # B: the masked round; "granted another replica" follows the deliveries
        eflags, granted, became = masked_round(o, G, P, np.nonzero(cand)[0].astype(np.int32), self.reach)
        self.ed[granted] = dl[granted]
        self.hd[became] = now + hb
        # C: local
        role1 = o.st["state"]
        elig = (role1 == LEADER) & (fired | became | bool(send_all))
        term = o.st["current_term"].astype(np.int64)
        key = np.where(elig, term * 8 + (7 - slots % P), -1).reshape(G, P)
        best = key.argmax(axis=1)
        has = key.max(axis=1) >= 0
        lp = np.where(has, best, -1).astype(np.int32)
        sender = (np.arange(G) * P + np.maximum(lp, 0))
        tg = np.where(has, term[sender], 0)
        self.hd[sender[has]] = now + hb
        self.stats["grants"] += int(granted.sum())
        self.stats["elected"] += int(became.sum())
        # D: the masked tick
        self.tick_record = {}
        gf = masked_tick(o, lp, self.reach, self.tick_record)
        commit, tl = o.export_group_status(lp)
        # E: a non-sender heard the sender only when both their bits are set
        conn = connected(self.reach, G, P)
        live = ((gf & _abi.G_ACTIVE) != 0) & ((gf & _abi.G_ERROR) == 0)
        term2 = o.st["current_term"].reshape(G, P)
        is_sender = np.arange(P)[None, :] == lp[:, None]
        heard = conn & conn[np.arange(G), np.maximum(lp, 0)][:, None]
        hit = live[:, None] & np.where(is_sender, ((gf & _abi.G_STEPPED_DOWN) != 0)[:, None],
                                       heard & (term2 == tg[:, None]))
        hit = hit.reshape(-1)
        self.ed[hit] = dl[hit]
        return dict(cand_mask=bits, leader_peer=lp, election_flags=eflags, group_flags=gf, commit=commit,
                    term_leader=tl)
