"""The host-driven sequence of one clock tick (include/mraft.h "timers": the
second way to run a deployment) and its comparison with mraft_clock_step.
Test infrastructure only.

host_sequence(node, now, send_all) drives `node` — an Engine, or the model's
ModelNode — through the message-level calls with mraft_timers_note after each:

 1. ticker(now) with full capacities: the election list E, the heartbeat list H.
 2. start_election(E); then, candidate rank by candidate rank within a group
    (distinct voter slots per call, as TimersModel._round batches them),
    handle_request_vote and timers_note(NOTE_RV_HANDLED).
 3. process_vote_replies in voter order, timers_note(NOTE_RV_FOLDED). With
    P = 1 only start_election runs.
 4. The sender of each group by the header's rule C: among the replicas that
    are Leader now and are in H, or became Leader in 3, or (send_all) simply
    hold office, the highest currentTerm, the lowest peer on a tie.
 5. For the senders' followers: gather_append_args (items with a gather error
    dropped), handle_append_entries by reference, timers_note(NOTE_AE_HANDLED),
    message_cases.results_of, process_append_replies,
    timers_note(NOTE_AE_FOLDED).

Where the two ways must agree. A group is INSIDE at a step when the clock
step's group_flags carry none of MRAFT_G_ERROR, MRAFT_G_NEED_SNAPSHOT,
MRAFT_G_LOG_FULL, MRAFT_G_FOLLOWER_PANIC and at most one replica is eligible in
rule C. That leaves out what the sequence above does not do or does in another
order: InstallSnapshot folded in peer order between the AppendEntries replies,
dropped messages (which step E of the clock step still resets, by its
documented rule), and two competing Leaders (the sequence sends for one). A
group counts as inside a case only if it is inside at every step of the case.

Inside groups are equal in every per-slot state array (persist bits among
them), in the logical logs and in election_due. heartbeat_due is equal except
at two kinds of slot, where both values are known:
 - a Leader that fired in A (it is in H) but is not the sender (deposed by the
   election round): the clock step leaves its timer due (heartbeat_due <= now,
   unchanged), the sequence's ticker reset it to now + heartbeat;
 - a sender that did not fire (newly elected, or send_all): the clock step
   resets it to now + heartbeat, the sequence leaves it unchanged unless
   NOTE_RV_FOLDED set it (then both are now + heartbeat).

After every step lockstep() copies the clock-step side's state and timers into
the sequence side, so a group that is outside cannot drift into the next step.
The clock-step side reloads that same image too, because load_state recomputes
terms_sorted: both sides start every step from a freshly loaded state. So this
comparison covers the clock step on loaded images only; consecutive clock
steps on a state that evolved on the device, with no reload in between, are
run_clock_case's (tests/test_timers_gpu.py, against the model).
"""
from __future__ import annotations

import numpy as np

from message_cases import all_follower_items, results_of
from multiraft_amd import _abi
from multiraft_amd._abi import (LEADER, NOTE_AE_FOLDED, NOTE_AE_HANDLED, NOTE_RV_FOLDED, NOTE_RV_HANDLED,
                                RV_ARGS, RV_RESULT)
from oracle_lib import assert_states_equal
from timers_cases import CFG, CLOCK_STEPS, NOW0, clock_case_model
from timers_model import ModelNode

OUTSIDE_FLAGS = _abi.G_ERROR | _abi.G_NEED_SNAPSHOT | _abi.G_LOG_FULL | _abi.G_FOLLOWER_PANIC


def host_sequence(node, now, send_all=False):
    """One tick of the host-driven sequence on `node`. Returns what happened:
    E, H (the ticker's lists), granted / became / stepped_down / deposed
    (bool[G*P]: voters that granted, replicas elected in 3, senders whose fold
    stepped down, replicas in H that are no longer Leader after 3),
    leader_peer[G] and n_eligible[G] of rule C."""
    G, P = node.G, node.P
    gp = G * P
    E, n_e, H, n_h = node.ticker(now)
    assert (n_e, n_h) == (len(E), len(H))
    granted, became, stepped = np.zeros(gp, bool), np.zeros(gp, bool), np.zeros(gp, bool)
    if len(E):                                                       # 2
        args, err = node.start_election(E)
        assert not err.any()
    if len(E) and P >= 2:
        grp = E // P
        rank = np.arange(len(E)) - np.searchsorted(grp, grp)         # rank among its group's candidates
        res = np.zeros((len(E), P), dtype=RV_RESULT)
        for k in range(int(rank.max()) + 1):
            idx = np.nonzero(rank == k)[0]
            src = np.repeat(idx, P - 1)
            q = np.tile(np.arange(P - 1), len(idx))
            vp = np.where(q < E[src] % P, q, q + 1)                  # every peer but the candidate
            a = np.zeros(len(src), dtype=RV_ARGS)
            a["slot"] = (E[src] // P) * P + vp
            a["candidate_id"] = E[src] % P
            for f in ("term", "last_log_index", "last_log_term"):
                a[f] = args[f][src]
            rep, herr = node.handle_request_vote(a)
            assert not herr.any()
            node.timers_note(NOTE_RV_HANDLED, a, rep, herr, now)
            granted[a["slot"][rep["vote_granted"] != 0]] = True
            r = np.zeros(len(src), dtype=RV_RESULT)
            r["slot"], r["peer"], r["args_term"] = E[src], vp, a["term"]
            r["reply_term"], r["vote_granted"] = rep["term"], rep["vote_granted"]
            res[src, vp] = r
        items = res[np.arange(P)[None, :] != (E % P)[:, None]]       # 3: voter order within each candidate
        seg = np.arange(len(E) + 1, dtype=np.int64) * (P - 1)
        fl, terr = node.process_vote_replies(items, seg)
        assert not terr.any()
        node.timers_note(NOTE_RV_FOLDED, items, fl, terr, now)
        became[items["slot"][(fl & _abi.F_BECAME_LEADER) != 0]] = True
    st = node.scalar_state()                                         # 4
    role, term = np.array(st["state"]), np.array(st["current_term"]).astype(np.int64)
    fired = np.zeros(gp, bool)
    fired[H] = True
    elig = ((role == LEADER) & (fired | became | bool(send_all))).reshape(G, P)
    t = np.where(elig, term.reshape(G, P), -1)
    lp = np.where(elig.any(axis=1), (t == t.max(axis=1, keepdims=True)).argmax(axis=1), -1).astype(np.int32)
    slots, peers = all_follower_items(lp, G, P)                      # 5
    if len(slots):
        args, gerr = node.gather_append_args(slots, peers)
        ok = gerr == 0
        args, slots, peers = args[ok], slots[ok], peers[ok]
    if len(slots):
        rep, herr = node.handle_append_entries(args, None)
        node.timers_note(NOTE_AE_HANDLED, args, rep, herr, now)
        res, seg = results_of(slots, peers, args, rep, herr, G, P)
        if len(res):
            fl, ferr = node.process_append_replies(res, seg)
            node.timers_note(NOTE_AE_FOLDED, res, fl, ferr, now)
            stepped[res["slot"][(fl & _abi.F_STEPPED_DOWN) != 0]] = True
    return dict(E=E, H=H, granted=granted, became=became, stepped_down=stepped, deposed=fired & (role != LEADER),
                leader_peer=lp, n_eligible=elig.sum(axis=1))


def lockstep(clock, seq, now0, steps, send_all):
    """`steps` ticks from now0: clock.clock_step next to host_sequence(seq),
    both from the same state and timers. Returns one record per step (the
    outputs, both sides' state and timers afterwards, heartbeat_due before)."""
    recs = []
    for k in range(steps):
        now = now0 + k
        hd0 = clock.timers_store()[1].copy()
        out = clock.clock_step(now, send_all)
        info = host_sequence(seq, now, send_all)
        cs, ct = clock.store_state(), clock.timers_store()
        recs.append(dict(now=now, hd0=hd0, out=out, info=info, clock=(cs,) + tuple(ct),
                         seq=(seq.store_state(),) + tuple(seq.timers_store())))
        # load_state recomputes terms_sorted (a proof the engine keeps, 0 = not
        # known), so the clock side reloads its own image too: both sides
        # start every step from the same loaded state
        clock.load_state(cs)
        seq.load_state(cs)
        seq.timers_load(*ct)
    return recs


def inside_groups(recs):
    """bool[G]: the groups that are inside at every step."""
    ins = None
    for r in recs:
        now_in = ((r["out"]["group_flags"] & OUTSIDE_FLAGS) == 0) & (r["info"]["n_eligible"] <= 1)
        ins = now_in if ins is None else ins & now_in
    return ins


def restrict(st, groups, P):
    """The state image of the groups `groups` (bool[G]) only."""
    slot = np.repeat(groups, P)
    return {k: v[np.repeat(slot, len(v) // len(slot))] for k, v in st.items()}


def compare(recs, G, P, L, heartbeat, ctx=""):
    """The comparison the module's docstring defines, over the groups that are
    inside at every step. Returns counts: inside groups, the heartbeat_due
    differences of the two kinds, and how often the inside groups saw a grant,
    an election, a sender stepping down and a fired Leader deposed."""
    ins = inside_groups(recs)
    slot_in = np.repeat(ins, P)
    n_in = int(ins.sum())
    stats = dict(groups=G, inside=n_in, hd_fired_not_sender=0, hd_sender_not_fired=0, grants=0, elected=0,
                 sender_stepped_down=0, fired_deposed=0)
    for k, r in enumerate(recs):
        c = f"{ctx} step {k}"
        now, info = r["now"], r["info"]
        (cs, ced, chd), (ss, sed, shd) = r["clock"], r["seq"]
        if n_in:
            assert_states_equal(restrict(cs, ins, P), restrict(ss, ins, P), n_in, P, L, c + " (inside groups)")
        lp = r["out"]["leader_peer"]
        assert np.array_equal(lp[ins], info["leader_peer"][ins]), c
        bad = np.nonzero(slot_in & (ced != sed))[0]
        assert not len(bad), f"{c}: election_due differs at {bad[:8]}: {ced[bad[:8]]} vs {sed[bad[:8]]}"
        fired = np.zeros(G * P, bool)
        fired[info["H"]] = True
        sender = np.zeros(G * P, bool)
        sender[(np.arange(G) * P + lp)[lp >= 0]] = True
        k1 = slot_in & fired & ~sender
        k2 = slot_in & sender & ~fired
        rest = slot_in & ~k1 & ~k2
        bad = np.nonzero(rest & (chd != shd))[0]
        assert not len(bad), f"{c}: heartbeat_due differs at {bad[:8]}: {chd[bad[:8]]} vs {shd[bad[:8]]}"
        # a Leader that fired and is not the sender: still due / reset by the ticker
        assert np.array_equal(chd[k1], r["hd0"][k1]) and (chd[k1] <= now).all(), c
        assert (shd[k1] == now + heartbeat).all(), c
        # a sender that did not fire: reset / untouched unless it was just elected
        assert (chd[k2] == now + heartbeat).all(), c
        assert np.array_equal(shd[k2], np.where(info["became"][k2], now + heartbeat, r["hd0"][k2])), c
        stats["hd_fired_not_sender"] += int((k1 & (chd != shd)).sum())
        stats["hd_sender_not_fired"] += int((k2 & (chd != shd)).sum())
        for name, key in (("grants", "granted"), ("elected", "became"), ("sender_stepped_down", "stepped_down"),
                          ("fired_deposed", "deposed")):
            stats[name] += int((info[key] & slot_in).sum())
    return stats


def model_pair(P, G, send_all):
    """(L, clock-step side, sequence side): two models of one clock case
    (tests/timers_cases.py)."""
    L, _, _, _, m1 = clock_case_model(P, G, send_all)
    m2 = clock_case_model(P, G, send_all)[-1]
    return L, ModelNode(m1), ModelNode(m2)


def run_model_case(P, G, send_all):
    """The model's clock step next to the sequence on a second model, compared:
    (records, counts)."""
    L, a, b = model_pair(P, G, send_all)
    recs = lockstep(a, b, NOW0, CLOCK_STEPS, send_all)
    return recs, compare(recs, G, P, L, CFG["heartbeat"], f"model, P {P} G {G} send_all {send_all}")
