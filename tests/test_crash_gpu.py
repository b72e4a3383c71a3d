"""The in-place crash (mraft_crash) on libmraft_hip.so against the model of
tests/crash_model.py: the reset, proof and broken-bounds families of
tests/crash_cases.py in this process and in a child on the small-grid
library, the timers of a replica that is down, crash + timers_arm against the
host round trip it replaces (read_persistent -> restore -> timers_arm) under
every tick mode and shard count, a down replica across 2 * election_hi clock
steps, device-resident batches, and the reference's crash tests
(TestPersist12C / 22C / 32C, TestFigure82C) on the co-resident path. The cases'
cells are proved present by tests/test_crash_cases.py. Every comparison with
the model is taken with heads=False (its restore starts a new ring); that the
engine moved no term is checked on its raw log array around every crash call."""
import os

import numpy as np
import pytest

import crash_cases as cc
from crash_model import CrashModel, assert_log_untouched
from gpu_support import behind_spin, run_cases_child
from oracle_lib import assert_states_equal
from reach_model import connected
from timers_cases import CFG, NOW0, clock_case
from timers_model import restart

from multiraft_amd import Engine, _abi, features
from multiraft_amd._abi import DEVICE, HOST, LEADER, TICK_AUTO, TICK_FULL, TICK_LIGHT, TIMER_NEVER, ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID1 = os.path.join(ROOT, "multiraft_amd", "libmraft_hip_grid1.so")
CLOCK_OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


def test_feature_bit_and_argument_checks_gpu():
    assert features() & _abi.FEATURE_CRASH
    lib = _abi.lib()
    G, P, L = 4, 3, 16
    with Engine(G, P, L) as e:
        assert lib.mraft_crash(e._h, None, 0, None, HOST) == _abi.OK      # n == 0 with NULL pointers
        assert lib.mraft_crash(e._h, None, 0, None, DEVICE) == _abi.OK
        assert lib.mraft_crash(e._h, None, 1, None, HOST) == _abi.E_INVAL
        assert lib.mraft_crash(e._h, None, -1, None, HOST) == _abi.E_INVAL
        assert len(e.crash(np.zeros(0, np.int32))) == 0
    with Engine(G, P, L, alloc=False) as e:                               # no state bound
        s = np.zeros(1, np.int32)
        assert lib.mraft_crash(e._h, ptr(s), 1, None, HOST) == _abi.E_NOSTATE


@pytest.mark.parametrize("name", cc.NAMES)
def test_family_gpu(name):
    assert cc.run_family(name, Engine) == cc.n_items(name)


def test_small_grid_library_child_gpu():
    """Every family in a fresh process on the small-grid library."""
    out = run_cases_child(os.path.join(ROOT, "tests", "crash_cases.py"), GRID1)
    assert [c[0] for c in out["cases"]] == cc.NAMES, out["cases"]
    assert all(c[2] is True and c[1] == cc.n_items(c[0]) for c in out["cases"]), out["cases"]


# ---- timers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R3_16", "R8_13"])
def test_timers_of_a_down_replica_gpu(name):
    """Enabled: both deadlines of every crashed replica are TIMER_NEVER and no
    other deadline moves. Disabled again: the call is the state part only."""
    fam = cc.family(name)
    G, P, L = fam["G"], fam["P"], fam["L"]
    slots = fam["batches"][5][0]
    with Engine(G, P, L) as e:
        e.load_state(fam["st"])
        m = CrashModel(G, P, L, fam["st"])
        e.timers_enable(7, 3, 10, 30, 5)
        m.enable(7, 3, 10, 30, 5)
        ed0, hd0 = e.timers_store()
        before = e.store_state()
        err, want = e.crash(slots), m.crash(slots)
        assert np.array_equal(err, want)
        ed, hd = e.timers_store()
        good = cc.good_slots(slots, want)
        assert (ed[good] == TIMER_NEVER).all() and (hd[good] == TIMER_NEVER).all() and len(good) > 32
        assert np.array_equal(ed, m.ed) and np.array_equal(hd, m.hd)
        rest = np.ones(G * P, bool)
        rest[good] = False
        assert np.array_equal(ed[rest], ed0[rest]) and np.array_equal(hd[rest], hd0[rest])
        after = e.store_state()
        assert_states_equal(after, m.state(), G, P, L, name, heads=False)
        assert_log_untouched(before, after, name)
        e.timers_arm(good, 9)                                             # start1: Make's two timers
        m.arm(good, 9)
        ed, hd = e.timers_store()
        assert np.array_equal(ed, m.ed) and np.array_equal(hd, m.hd) and (ed[good] < 9 + 30).all()
        e.timers_disable()
        e.load_state(fam["st"])
        assert np.array_equal(e.crash(slots), want)
        assert_states_equal(e.store_state(), m.state(), G, P, L, name + ", timers disabled", heads=False)


# ---- the round trip it replaces ---------------------------------------------------------------------
@pytest.mark.parametrize("shards", (1, 2))
@pytest.mark.parametrize("mode", [TICK_FULL, TICK_LIGHT, TICK_AUTO])
def test_crash_and_arm_equals_the_host_round_trip_gpu(mode, shards):
    """One engine crashes in place and arms; a second goes through
    read_persistent -> restore -> timers_arm (timers_model.restart) on the same
    slots: equal but for the ring heads, and still equal after three clock steps."""
    leaders = heads_differ = 0
    for P, G, sa in ((3, 33, False), (5, 33, False), (8, 33, True)):     # the tick fuzz generator's states
        L, st, ed, hd = clock_case(P, G, sa)
        n = st["last_index"].astype(np.int64) - st["dummy_index"]
        ok = (n >= 0) & (n < L) & (st["dummy_index"] >= 0)
        pick = ok & ((st["state"] == LEADER) | (np.arange(G * P) % 3 == 1))
        slots = np.nonzero(pick)[0].astype(np.int32)
        assert len(slots) > G
        leaders += int((st["state"][slots] == LEADER).sum())
        with Engine(G, P, L) as a, Engine(G, P, L) as b:
            for x in (a, b):
                x.load_state(st)
                x.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
                x.timers_load(ed, hd)
                x.set_tick_mode(mode)
                if shards > 1:
                    x.set_tick_shards(shards)
            before = a.store_state()
            assert not a.crash(slots).any()
            mid = a.store_state()
            assert_log_untouched(before, mid, "in place")
            a.timers_arm(slots, NOW0)
            restart(b, slots, NOW0)
            for k in range(4):
                ctx = f"P {P} mode {mode} shards {shards} after {k} steps"
                assert_states_equal(a.store_state(), b.store_state(), G, P, L, ctx, heads=False)
                for x, y in zip(a.timers_store(), b.timers_store()):
                    assert np.array_equal(x, y), ctx
                if k < 3:
                    oa, ob = a.clock_step(NOW0 + k, True), b.clock_step(NOW0 + k, True)
                    for nme in CLOCK_OUTS:
                        assert np.array_equal(oa[nme], ob[nme]), (ctx, nme)
            heads_differ += int((mid["log_head"][slots] != b.store_state()["log_head"][slots]).sum())
    assert leaders > 64 and heads_differ > 64      # Leaders crashed; rings the round trip moved and the call did not


# ---- a replica that is down ---------------------------------------------------------------------------
@pytest.mark.parametrize("P", (3, 5))
def test_down_replica_is_untouched_while_its_group_goes_on_gpu(P):
    """Crashed, its bit cleared: bit-identical in every array and both timers
    across 2 * election_hi clock steps, while its group elects and commits
    without it."""
    G, L, cfg = 64, cc.SCEN_L, cc.SCEN_CFG
    with Engine(G, P, L) as e:
        e.timers_enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], 0)
        t = 0
        for t in range(1, 2 * cfg["hi"] + 1):                             # every group elects
            if t % 4 == 0:
                s = np.nonzero(e.scalar_state()["state"] == LEADER)[0].astype(np.int32)
                e.start(s, np.ones(len(s), np.int32))
            e.clock_step(t, True)
        st = e.store_state()
        role = st["state"].reshape(G, P)
        assert ((role == LEADER).sum(axis=1) == 1).all()
        lead = np.array([int(np.nonzero(r == LEADER)[0][0]) for r in role])
        # the Leader in even groups, the follower after it in odd ones
        down = np.arange(G) * P + (lead + np.arange(G) % 2) % P
        assert not e.crash(down.astype(np.int32)).any()
        reach = (np.full(G, (1 << P) - 1) & ~(1 << (down % P))).astype(np.uint8)
        e.set_reachable(reach)
        st0, (ed0, hd0) = e.store_state(), e.timers_store()
        assert (ed0[down] == TIMER_NEVER).all() and (hd0[down] == TIMER_NEVER).all()
        assert (st0["state"][down] == _abi.FOLLOWER).all()
        commit0 = st0["commit_index"].reshape(G, P).max(axis=1)
        for t in range(t + 1, t + 2 * cfg["hi"] + 1):
            if t % 4 == 0:
                s = np.nonzero(e.scalar_state()["state"] == LEADER)[0].astype(np.int32)
                e.start(s, np.ones(len(s), np.int32))
            e.clock_step(t, True)
        st1, (ed1, hd1) = e.store_state(), e.timers_store()
        for k in st0:
            rows = G * P
            assert np.array_equal(st1[k].reshape(rows, -1)[down], st0[k].reshape(rows, -1)[down]), (k, "a down replica changed")
        assert np.array_equal(ed1[down], ed0[down]) and np.array_equal(hd1[down], hd0[down])
        up = connected(reach, G, P)
        role1 = st1["state"].reshape(G, P)
        assert (((role1 == LEADER) & up).sum(axis=1) == 1).all(), "a Leader among the replicas that are up"
        assert (st1["commit_index"].reshape(G, P).max(axis=1) > commit0).all(), "the group commits without it"
        # start1: it comes back and catches up
        e.timers_arm(down.astype(np.int32), t)
        e.set_reachable(None)
        for t in range(t + 1, t + cfg["hi"] + 1):
            e.clock_step(t, True)
        st2 = e.store_state()
        assert (st2["commit_index"][down] >= st1["commit_index"].reshape(G, P).max(axis=1)).all()


# ---- device buffers -------------------------------------------------------------------------------------
def test_device_buffers_back_to_back_gpu():
    """Two calls with MRAFT_DEVICE buffers enqueued behind a device spin, timers
    enabled, the second with item_err NULL: nothing waits for the device."""
    import torch
    fam = cc.family("R5_16")
    G, P, L = fam["G"], fam["P"], fam["L"]
    sa, sb = fam["batches"][4][0], fam["batches"][6][0]
    dev = torch.device("cuda", 0)
    da, db = (torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in (sa, sb))
    ea = torch.full((len(sa),), -1, dtype=torch.int32, device=dev)
    m = CrashModel(G, P, L, fam["st"])
    m.enable(7, 3, 10, 30, 0)
    with Engine(G, P, L) as e:
        e.load_state(fam["st"])
        e.timers_enable(7, 3, 10, 30, 0)
        before = e.store_state()
        with behind_spin(e, what="mraft_crash with device buffers"):
            assert e.crash(da, where=DEVICE, out=(ea,)) is ea
            assert e.crash(db, where=DEVICE, out=(None,)) is None
        wa = m.crash(sa)
        m.crash(sb)
        assert np.array_equal(ea.cpu().numpy(), wa)
        after = e.store_state()
        assert_states_equal(after, m.state(), G, P, L, "two device calls back to back", heads=False)
        assert_log_untouched(before, after, "two device calls")
        for x, y in zip(e.timers_store(), (m.ed, m.hd)):
            assert np.array_equal(x, y)


# ---- the reference's crash tests on the co-resident path --------------------------------------------------
@pytest.mark.parametrize("P", (3, 5))
def test_crash_scenarios_gpu(P):
    """TestPersist12C and TestPersist32C (P = 3), TestPersist22C and
    TestFigure82C (P = 5) (src/raft/test_test.go:685-871), one per group, each
    group's schedule shifted by its index, on 64 groups: engine and model in
    lockstep."""
    with Engine(64, P, cc.SCEN_L) as e:
        c = cc.run_scenarios(P, 64, e)
    assert c["majority_leader"] > 64 and c["agree"] > 64 and c["no_quorum"] > 0, c
    assert c["crashes"] > 64 and c["restarts"] > 64 and c["leader_crashed"] > 32 and c["reapplied"] > 64, c
