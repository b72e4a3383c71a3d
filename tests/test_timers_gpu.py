"""The device-resident timers against the numpy model (tests/timers_model.py),
through the C ABI: enable / arm / load / store, mraft_ticker (counts, caps and
remainders), mraft_timers_note for the six reset sites on real outputs of the
message path, mraft_clock_step on arbitrary states, and the self-driving run
(test_test.go TestInitialElection / TestReElection). After every call the
whole state and both timer arrays equal the model's. The tests of sections
1-3 and the CLOCK_CASES assert no tick mode and pass under every one; the
clock step also runs under each mode set by the test, with 1, 2 and 3 tick
shards (section 4b), and the self-driving run under MRAFT_TICK_LIGHT."""
import ctypes

import numpy as np
import pytest

from message_cases import all_follower_items, external_entries, results_of
from oracle_lib import assert_states_equal
from random_states import random_tick_state
from timers_cases import CFG, CLOCK_CASES, CLOCK_STEPS, NOW0, clock_case_model, due_timers, leaders_in_place_state
from timers_model import SELF_CFG, SELF_L, SELF_SHAPES, ModelNode, TimersModel, self_driving

from multiraft_amd import Engine, _abi, new_state
from multiraft_amd._abi import (HOST, IS_RESULT, LEADER, NOTE_AE_FOLDED, NOTE_AE_HANDLED, NOTE_IS_FOLDED,
                                NOTE_IS_HANDLED, NOTE_RV_FOLDED, NOTE_RV_HANDLED, RV_ARGS, RV_RESULT, ptr)

pytestmark = pytest.mark.gpu

OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


def same(e: Engine, m: TimersModel, ctx, state=True):
    if state:
        assert_states_equal(e.store_state(), m.state(), e.G, e.P, e.L, ctx)
    ed, hd = e.timers_store()
    for name, a, b in (("election_due", ed, m.ed), ("heartbeat_due", hd, m.hd)):
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0][:8]
            raise AssertionError(f"{ctx}: {name} differs at {bad}: {a[bad]} vs {b[bad]}")


def enable_both(e, m, cfg=CFG, now=0):
    e.timers_enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], now)
    m.enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], now)


def load_both(e, m, ed=None, hd=None):
    e.timers_load(ed, hd)
    m.load(ed, hd)


# ---- 1. enable, arm, load and store ---------------------------------------------------

@pytest.mark.parametrize("G,P,L", [(1, 1, 1), (33, 5, 8), (257, 3, 8)])
def test_enable_arm_load_store(G, P, L):
    lib = _abi.lib()
    rng = np.random.default_rng(G)
    gp = G * P
    m = TimersModel(G, P, L)
    buf, n64 = np.zeros(gp, np.int32), np.zeros(1, np.int64)
    soa = _abi.MraftTimersSoa(ptr(buf), ptr(buf))
    cfg = _abi.MraftTimerConfig(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"])

    def every_other_call(h):
        return [lib.mraft_timers_disable(h), lib.mraft_timers_load(h, ctypes.byref(soa), HOST),
                lib.mraft_timers_store(h, ctypes.byref(soa), HOST), lib.mraft_timers_arm(h, ptr(buf), 1, 0, HOST),
                lib.mraft_ticker(h, 0, ptr(buf), gp, ptr(n64), ptr(buf), gp, ptr(n64), HOST),
                lib.mraft_timers_note(h, NOTE_AE_FOLDED, ptr(buf), ptr(buf), None, 0, 0, HOST),
                lib.mraft_clock_step(h, 0, 0, None, None, None, None, None, None, HOST)]

    with Engine(G, P, L) as e:
        h = e._h
        assert every_other_call(h) == [_abi.E_NOSTATE] * 7
        assert b"not enabled" in lib.mraft_last_error_string()
        for bad in ((0, 6, 14, 0), (4, 0, 14, 0), (4, 14, 14, 0), (4, 6, (1 << 20) + 1, 0), (4, 6, 14, -1),
                    (4, 6, 14, (1 << 30) + 1)):
            c = _abi.MraftTimerConfig(1, bad[0], bad[1], bad[2])
            assert lib.mraft_timers_enable(h, ctypes.byref(c), bad[3]) == _abi.E_INVAL, bad
        assert lib.mraft_timers_enable(h, None, 0) == _abi.E_INVAL
        assert lib.mraft_timers_store(h, ctypes.byref(soa), HOST) == _abi.E_NOSTATE  # a rejected enable enables nothing
        enable_both(e, m, now=5)
        same(e, m, "enable")
        assert (m.ed > 5 + CFG["lo"] - 1).all() and (m.ed < 5 + CFG["hi"]).all() and (m.hd == 5 + CFG["heartbeat"]).all()
        # arm: a subset, a repeated slot, out-of-range slots skipped
        slots = np.concatenate([rng.integers(0, gp, size=max(1, gp // 3)), [-1, gp, gp + 7, 0, 0]]).astype(np.int32)
        e.timers_arm(slots, 17)
        m.arm(slots, 17)
        same(e, m, "arm")
        assert lib.mraft_timers_arm(h, ptr(slots), len(slots), -1, HOST) == _abi.E_INVAL
        # load / store: both arrays, then one of them only
        ed, hd = due_timers(rng, gp, 40, 0.5), due_timers(rng, gp, 50, 0.5)
        load_both(e, m, ed, hd)
        same(e, m, "load")
        load_both(e, m, ed=ed[::-1].copy())
        same(e, m, "load election_due only")
        got = e.timers_store()
        assert np.array_equal(got[0], ed[::-1]) and np.array_equal(got[1], hd)
        # enabling again re-arms under the new configuration
        cfg2 = dict(seed=9, heartbeat=50, lo=150, hi=300)
        enable_both(e, m, cfg2, now=1 << 30)
        same(e, m, "re-enable")
        assert lib.mraft_clock_step(h, (1 << 30) + 1, 0, None, None, None, None, None, None, HOST) == _abi.E_INVAL
        assert lib.mraft_clock_step(h, 0, 2, None, None, None, None, None, None, HOST) == _abi.E_INVAL
        e.timers_disable()
        assert every_other_call(h) == [_abi.E_NOSTATE] * 7
        enable_both(e, m, now=0)
        same(e, m, "enable after disable")
        assert lib.mraft_timers_enable(h, ctypes.byref(cfg), 0) == _abi.OK


# ---- 2. mraft_ticker ---------------------------------------------------------------------

# G*P in {1, 255, 257, 1,285}, and 262,155 slots: 1,025 blocks of 256, one past
# the 1,024 block counts the scan takes per chunk
@pytest.mark.parametrize("G,P,L", [(1, 1, 4), (51, 5, 4), (257, 1, 4), (257, 5, 8), (52431, 5, 4)])
def test_ticker(G, P, L):
    rng = np.random.default_rng(100 + G)
    gp = G * P
    st = leaders_in_place_state(G, P, L, rng, seed=700 + G)
    m = TimersModel(G, P, L, st)
    now = 500
    with Engine(G, P, L) as e:
        e.load_state(st)
        enable_both(e, m)

        def tick(now, cap_e, cap_h, ctx):
            got = e.ticker(now, cap_e, cap_h)
            want = m.ticker(now, cap_e, cap_h)
            for a, b, what in zip(got, want, ("election slots", "n_e", "heartbeat slots", "n_h")):
                assert np.array_equal(a, b), (ctx, what)
            assert (np.diff(got[0]) > 0).all() and (np.diff(got[2]) > 0).all(), ctx
            same(e, m, ctx, state=(gp < 10000))
            return got

        for share in (0.0, 0.5, 1.0):
            # capacities that cut the lists one short of full, after the first slot (mid-wave, in the first
            # block) and in the middle (mid-block, and for 262,155 slots past the scan's first chunk)
            for cut in ("n - 1", "1", "n // 2"):
                load_both(e, m, due_timers(rng, gp, now, share), due_timers(rng, gp, now, share))
                leader = st["state"] == LEADER
                full_e, full_h = np.nonzero((m.ed <= now) & ~leader)[0], np.nonzero((m.hd <= now) & leader)[0]
                _, ne, _, nh = tick(now, 0, 0, f"share {share}, cap 0")
                assert (ne, nh) == (len(full_e), len(full_h))
                # nothing was written, so every listed slot is still due; fewer than fit ...
                ce, ch = {"n - 1": (max(ne - 1, 0), max(nh - 1, 0)), "1": (min(1, ne), min(1, nh)),
                          "n // 2": (ne // 2, nh // 2)}[cut]
                e1, ne1, h1, nh1 = tick(now, ce, ch, f"share {share}, cap {cut}")
                assert (ne1, nh1, len(e1), len(h1)) == (ne, nh, ce, ch)
                assert np.array_equal(e1, full_e[:ce]) and np.array_equal(h1, full_h[:ch])
                # ... the slots past the cut are still due, the written ones are not ...
                ed, hd = e.timers_store()
                assert (ed[full_e[ce:]] <= now).all() and (ed[full_e[:ce]] > now).all(), (share, cut)
                assert (hd[full_h[ch:]] <= now).all() and (hd[full_h[:ch]] > now).all(), (share, cut)
                # ... and the second call returns exactly the remainder
                e2, ne2, h2, nh2 = tick(now, gp, gp, f"share {share}, cap {cut}, remainder")
                assert (ne2, nh2) == (ne - ce, nh - ch)
                assert np.array_equal(e2, full_e[ce:]) and np.array_equal(h2, full_h[ch:])
                assert tick(now, gp, gp, f"share {share}, cap {cut}, nothing left")[1::2] == (0, 0)
                now += 3
            load_both(e, m, due_timers(rng, gp, now, share), due_timers(rng, gp, now, share))
            tick(now, gp + 5, gp + 5, f"share {share}, cap >= n")
            now += 3
        if share == 1.0:
            assert ne + nh == gp  # every slot was in one list
        assert_states_equal(e.store_state(), m.state(), G, P, L, "ticker leaves the state alone")


# ---- 3. mraft_timers_note ------------------------------------------------------------------

@pytest.mark.parametrize("P,seed", [(3, 1), (5, 2)])
def test_timers_note_all_kinds(P, seed):
    """Every kind on real outputs of the message path (the engine's, equal to
    the oracle's): stale AppendEntries, the prev < dummy reply with term 0,
    rejected items, refused and granted votes, folds that step down, tallies
    that elect and that step down, duplicate slots in one batch."""
    rng = np.random.default_rng(3300 + seed)
    G, L = 300, 32
    st, lp = random_tick_state(rng, G, P, L, snap=True)
    lp = np.where((lp >= 0) & (lp < P), lp, 0).astype(np.int32)
    m = TimersModel(G, P, L, st)
    o = m.o
    seen = {}
    with Engine(G, P, L) as e:
        e.load_state(st)
        enable_both(e, m)

        def note(kind, rec, out, err, now, ctx):
            e.timers_note(kind, rec, out, err, now)
            m.note(kind, rec, out, err, now)
            same(e, m, ctx)

        slots, peers = all_follower_items(lp, G, P)
        # --- InstallSnapshot: gather, handle, fold
        ia, ierr = e.gather_install_snapshot_args(slots, peers)
        oa, oerr = o.gather_install_snapshot_args(slots, peers)
        assert np.array_equal(ia, oa) and np.array_equal(ierr, oerr)
        pick = (ierr == 0) & (ia["slot"] >= 0)
        ia, isl, ipe = ia[pick], slots[pick], peers[pick]
        ia = np.concatenate([ia, ia[:5]])  # repeated receivers: rejected (item_err != 0)
        isl, ipe = np.concatenate([isl, isl[:5]]), np.concatenate([ipe, ipe[:5]])
        rep, fl, herr = e.handle_install_snapshot(ia)
        orep, ofl, oherr = o.handle_install_snapshot(ia)
        assert np.array_equal(rep, orep) and np.array_equal(herr, oherr)
        seen["is_rejected"] = int((herr != 0).sum())
        seen["is_stale"] = int(((herr == 0) & (rep["term"] > ia["term"])).sum())
        seen["is_reset"] = int(((herr == 0) & (rep["term"] <= ia["term"])).sum())
        note(NOTE_IS_HANDLED, ia, rep, herr, 11, "IS handled")
        ok = herr == 0
        res = np.zeros(int(ok.sum()), dtype=IS_RESULT)
        res["slot"], res["peer"], res["args_term"] = isl[ok], ipe[ok], ia["term"][ok]
        res["args_last_included_index"], res["reply_term"] = ia["last_included_index"][ok], rep["term"][ok]
        order = np.argsort(res["slot"], kind="stable")
        res = res[order]
        seg = np.concatenate([[0], np.nonzero(np.diff(res["slot"]))[0] + 1, [len(res)]]).astype(np.int64)
        ffl, ferr = e.process_install_snapshot_replies(res, seg)
        offl, oferr = o.process_install_snapshot_replies(res, seg)
        assert np.array_equal(ffl, offl) and np.array_equal(ferr, oferr)
        seen["is_fold_stepdown"] = int((ffl & _abi.F_STEPPED_DOWN).astype(bool).sum())
        note(NOTE_IS_FOLDED, res, ffl, ferr, 12, "IS folded")
        # --- AppendEntries: gather, handle (by reference), fold
        aa, gerr = e.gather_append_args(slots, peers)
        oa, ogerr = o.gather_append_args(slots, peers)
        assert np.array_equal(aa, oa) and np.array_equal(gerr, ogerr)
        pick = gerr == 0
        aa, asl, ape = aa[pick], slots[pick], peers[pick]
        aa = np.concatenate([aa, aa[:7]])  # repeated receivers: MRAFT_ITEM_DUP_SLOT
        asl, ape = np.concatenate([asl, asl[:7]]), np.concatenate([ape, ape[:7]])
        # the entries by value, as the network would deliver them
        xa, xbuf = external_entries(aa, np.ones(len(aa), bool), e.store_state(), L)
        rep, herr = e.handle_append_entries(xa, xbuf)
        orep, oherr = o.handle_append_entries(xa, xbuf)
        assert np.array_equal(rep, orep) and np.array_equal(herr, oherr)
        seen["ae_rejected"] = int((herr != 0).sum())
        seen["ae_dup"] = int((herr == _abi.ITEM_DUP_SLOT).sum())
        seen["ae_stale"] = int(((herr == 0) & (rep["term"] > aa["term"])).sum())
        seen["ae_term0"] = int(((herr == 0) & (rep["term"] == 0) & (aa["term"] > 0)).sum())
        seen["ae_reset"] = int(((herr == 0) & (rep["term"] <= aa["term"])).sum())
        note(NOTE_AE_HANDLED, xa, rep, herr, 13, "AE handled")
        res, seg = results_of(asl, ape, aa, rep, herr, G, P)
        ffl, ferr = e.process_append_replies(res, seg)
        offl, oferr = o.process_append_replies(res, seg)
        assert np.array_equal(ffl, offl) and np.array_equal(ferr, oferr)
        seen["ae_fold_stepdown"] = int((ffl & _abi.F_STEPPED_DOWN).astype(bool).sum())
        seen["fold_dup_slots"] = int(len(res) - len(np.unique(res["slot"])))
        note(NOTE_AE_FOLDED, res, ffl, ferr, 14, "AE folded")
        note(NOTE_AE_FOLDED, res, ffl, None, 15, "AE folded, item_err NULL")
        # --- RequestVote: one candidate per group (distinct voters), handle, tally
        role = m.state()["state"].reshape(G, P)
        cp = np.array([int(rng.choice(np.nonzero(role[g] != LEADER)[0])) if (role[g] != LEADER).any() else -1
                       for g in range(G)])
        cs = (np.arange(G) * P + cp)[cp >= 0].astype(np.int32)
        ra, serr = e.start_election(cs)
        ora, oserr = o.start_election(cs)
        assert np.array_equal(ra, ora) and not serr.any() and not oserr.any()
        q = np.tile(np.arange(P - 1), len(cs))
        src = np.repeat(np.arange(len(cs)), P - 1)
        vp = np.where(q < cs[src] % P, q, q + 1)
        va = np.zeros(len(src), dtype=RV_ARGS)
        va["slot"] = (cs[src] // P) * P + vp
        va["candidate_id"] = cs[src] % P
        for f in ("term", "last_log_index", "last_log_term"):
            va[f] = ra[f][src]
        va = np.concatenate([va, va[:3]])  # repeated voters: rejected
        va["slot"][-1] = G * P + 4          # and a slot out of range
        rep, herr = e.handle_request_vote(va)
        orep, oherr = o.handle_request_vote(va)
        assert np.array_equal(rep, orep) and np.array_equal(herr, oherr)
        seen["rv_granted"] = int(((herr == 0) & (rep["vote_granted"] != 0)).sum())
        seen["rv_refused"] = int(((herr == 0) & (rep["vote_granted"] == 0)).sum())
        seen["rv_rejected"] = int((herr != 0).sum())
        note(NOTE_RV_HANDLED, va, rep, herr, 16, "RV handled")
        n = len(src)
        res = np.zeros(n, dtype=RV_RESULT)
        res["slot"], res["peer"], res["args_term"] = cs[src], vp, va["term"][:n]
        res["reply_term"], res["vote_granted"] = rep["term"][:n], rep["vote_granted"][:n]
        seg = np.arange(len(cs) + 1, dtype=np.int64) * (P - 1)
        tfl, terr = e.process_vote_replies(res, seg)
        otfl, oterr = o.process_vote_replies(res, seg)
        assert np.array_equal(tfl, otfl) and np.array_equal(terr, oterr)
        seen["tally_elected"] = int((tfl & _abi.F_BECAME_LEADER).astype(bool).sum())
        seen["tally_stepdown"] = int((tfl & _abi.F_STEPPED_DOWN).astype(bool).sum())
        hd0 = m.hd.copy()
        note(NOTE_RV_FOLDED, res, tfl, terr, 17, "RV folded")
        assert int((m.hd != hd0).sum()) == seen["tally_elected"]  # the step-down resets nothing
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


# ---- 4. mraft_clock_step on arbitrary states ------------------------------------------------

def run_clock_case(P, G, send_all, where=HOST, shards=1, mode=None):
    L, st, ed, hd, m = clock_case_model(P, G, send_all)
    with Engine(G, P, L) as e:
        e.load_state(st)
        if shards > 1:
            e.set_tick_shards(shards)
        if mode is not None:
            e.set_tick_mode(mode)
            assert e.tick_mode() == mode
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
        e.timers_load(ed, hd)
        for k in range(CLOCK_STEPS):
            ctx = f"P {P} G {G} send_all {send_all} step {k}"
            want = m.clock_step(NOW0 + k, send_all)
            if where == HOST:
                got = e.clock_step(NOW0 + k, send_all)
            else:
                import torch
                dev = {n: torch.zeros(G, dtype=torch.uint8 if n == "cand_mask" else torch.int32, device="cuda")
                       for n in OUTS}
                # the fills run on torch's stream, the step on the engine's own non-blocking one: without
                # this a fill can land after the step's store into the same buffer
                torch.cuda.synchronize()
                e.clock_step(NOW0 + k, send_all, where=_abi.DEVICE, out=dev)
                e.synchronize()
                got = {n: v.cpu().numpy() for n, v in dev.items()}
            for n in OUTS:
                assert np.array_equal(got[n], want[n]), (ctx, n, np.nonzero(got[n] != want[n])[0][:8])
            same(e, m, ctx)
    return m.stats


@pytest.mark.parametrize("P,G,send_all", CLOCK_CASES)
def test_clock_step_arbitrary_states(P, G, send_all):
    run_clock_case(P, G, send_all)


def test_clock_step_device_buffers():
    stats = run_clock_case(5, 300, True, where=_abi.DEVICE)
    assert stats["two_leaders_equal"] and stats["fired_deposed"] and stats["need_snapshot"]


def test_clock_step_two_tick_shards():
    stats = run_clock_case(8, 300, False, shards=2)
    assert stats["sender_stepped_down"] and stats["need_snapshot"]


# 4b. Under the tick mode and the shard count the test sets. G = 33 with three
# shards and G = 300 with two give uneven ranges and ranges shorter than a wave
# of eight groups per segment; MRAFT_TICK_LIGHT feeds the light launch a
# device-written leader_peer with many -1 entries, and its group_flags (or its
# fallback's) feed step E.
@pytest.mark.parametrize("where", [HOST, _abi.DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("shards", [1, 2, 3])
@pytest.mark.parametrize("mode", [_abi.TICK_FULL, _abi.TICK_LIGHT, _abi.TICK_AUTO], ids=["full", "light", "auto"])
@pytest.mark.parametrize("P,G,send_all", [(2, 33, False), (5, 300, True), (8, 300, False)])
def test_clock_step_tick_modes_and_shards(P, G, send_all, mode, shards, where):
    run_clock_case(P, G, send_all, where=where, shards=shards, mode=mode)


def test_clock_step_optional_outputs():
    """Every output is optional: with none the step still does all its work."""
    P, G = 3, 300
    L, st, ed, hd, m = clock_case_model(P, G, True)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
        e.timers_load(ed, hd)
        for k in range(CLOCK_STEPS):
            m.clock_step(NOW0 + k, True)
            assert _abi.lib().mraft_clock_step(e._h, NOW0 + k, 1, None, None, None, None, None, None, HOST) == 0
            same(e, m, f"no outputs, step {k}")


# ---- 5. the self-driving run ---------------------------------------------------------------------

class EngineNode:
    def __init__(self, e):
        self.e = e
        self.read_persistent, self.restore, self.timers_arm, self.start = (e.read_persistent, e.restore,
                                                                           e.timers_arm, e.start)

    def clock_step(self, now, send_all=False):
        return self.e.clock_step(now, send_all)


def self_driving_case(G, P, shards=1, mode=None):
    """Returns the light tick's fallback counts read after each leg-3 step."""
    L = SELF_L
    m = TimersModel(G, P, L)
    fallbacks = []
    with Engine(G, P, L) as e:
        e.load_state(new_state(G, P, L))
        if shards > 1:
            e.set_tick_shards(shards)
        if mode is not None:
            e.set_tick_mode(mode)
        enable_both(e, m, dict(seed=SELF_CFG["seed"], heartbeat=SELF_CFG["heartbeat"], lo=SELF_CFG["lo"],
                               hi=SELF_CFG["hi"]))

        def check(t, outs):
            for n in OUTS:
                assert np.array_equal(outs[1][n], outs[0][n]), (t, n)
            same(e, m, f"tick {t}")
            if t > 300 + 2 * SELF_CFG["hi"]:
                fallbacks.append(e.tick_light_fallbacks())

        hist = self_driving([ModelNode(m), EngineNode(e)], G, P, check)
        assert len(hist) == 300 + 2 * SELF_CFG["hi"] + 40
        if P >= 2:
            assert (hist[max(hist)][0] == 1).all()
    return fallbacks


@pytest.mark.parametrize("G,P", SELF_SHAPES)
def test_self_driving_run(G, P):
    """From Make state the engine's history under clock steps alone — then a
    crash and restart of every Leader, then Starts at the Leaders — is the
    model's at every step (tests/test_timers_model.py checks what the model's
    history must satisfy)."""
    self_driving_case(G, P)


@pytest.mark.parametrize("G,P", [(64, 5), (64, 2)])
def test_self_driving_run_light_two_shards(G, P):
    """The same run under MRAFT_TICK_LIGHT with two tick shards. With Leaders
    in place and followers caught up the light launch settles groups itself:
    after a leg-3 step fewer than G groups fell back to the full tick, so step
    E consumed group_flags written by k_tick_lite, not only by its fallback."""
    fallbacks = self_driving_case(G, P, shards=2, mode=_abi.TICK_LIGHT)
    assert len(fallbacks) == 40 and min(fallbacks) >= 0, fallbacks
    assert min(fallbacks) < G, fallbacks
