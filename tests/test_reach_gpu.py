"""The co-resident calls under a reachability mask (mraft_set_reachable) on
libmraft_hip.so against the model of tests/reach_model.py, bit for bit: the
tick in every mode and shard count, the election round, the clock step, and the
reference's connect / disconnect scenarios driven by nothing but set_reachable,
start, clock_step and the compacted applier. The cases are
tests/reach_cases.py's; tests/test_reach_cases.py proves what they contain."""
import numpy as np
import pytest

import election_cases as ec
import reach_cases as rc
from oracle_lib import Oracle, assert_states_equal, logical_logs
from reach_model import ReachModel, connected, full_mask, masked_election_rounds, masked_tick
from timers_cases import CFG, CLOCK_CASES, NOW0

from multiraft_amd import Engine, _abi, features
from multiraft_amd._abi import DEVICE, HOST, LEADER, TICK_AUTO, TICK_FULL, TICK_LIGHT, ptr

pytestmark = pytest.mark.gpu

CLOCK_OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


def test_feature_bit_and_mask_round_trip_gpu():
    assert features() & _abi.FEATURE_REACH
    G, P, L = 9, 3, 16
    with Engine(G, P, L) as e:
        assert e.get_reachable() is None
        m = np.arange(G, dtype=np.uint8) * 29
        e.set_reachable(m)
        assert np.array_equal(e.get_reachable(), m)
        m2 = m[::-1].copy()
        e.set_reachable(m2)
        m2[:] = 0                                   # the engine keeps its own copy
        assert np.array_equal(e.get_reachable(), m[::-1])
        e.set_reachable(None)
        assert e.get_reachable() is None
    with Engine(G, P, L, alloc=False) as e:         # no state bound
        rc_ = _abi.lib().mraft_set_reachable(e._h, ptr(m), HOST)
        assert rc_ == _abi.E_NOSTATE


@pytest.mark.parametrize("ka", rc.known_answers(), ids=lambda k: k["name"])
def test_known_answers_gpu(ka):
    """The hand-derived answers of tests/reach_cases.py on the engine."""
    with Engine(ka["G"], ka["P"], ka["L"]) as e:
        e.load_state(ka["st"])
        e.set_reachable(np.array(ka["reach"], np.uint8))
        if ka["kind"] == "tick":
            gf = e.replicate_tick(np.array(ka["lp"], np.int32))
        else:
            gf = e.election_rounds(np.array([ka["cand"]], np.uint8))
        rc.check_known_answer(ka, gf, e.store_state())


# ---- the tick ------------------------------------------------------------------------------------
def run_tick(P, G, seed, kind, mode=TICK_FULL, shards=1, ticks=2, export=False, device=False):
    st, lp, reach, _ = rc.tick_case(P, G, seed, kind)
    L = rc.TICK_L
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.set_tick_mode(mode)
        if shards > 1:
            e.set_tick_shards(shards)
        if device:
            import torch
            e.set_reachable(torch.from_numpy(reach).cuda(), where=DEVICE)
        else:
            e.set_reachable(reach)
        for k in range(ticks):                      # the second tick runs on the evolved state
            ctx = f"tick P {P} G {G} seed {seed} {kind} mode {mode} shards {shards} tick {k}"
            want = masked_tick(o, lp, reach)
            if device:
                import torch
                dlp = torch.from_numpy(lp).cuda()
                dgf = torch.zeros(G, dtype=torch.int32, device="cuda")
                e.replicate_tick(dlp, dgf, where=DEVICE)
                e.synchronize()
                got = dgf.cpu().numpy()
            elif export:
                got, c, tl = e.replicate_tick_export(lp)
                wc, wtl = o.export_group_status(lp)
                assert np.array_equal(c, wc) and np.array_equal(tl, wtl), (ctx, "export words")
            else:
                got = e.replicate_tick(lp)
            assert np.array_equal(got, want), (ctx, np.nonzero(got != want)[0][:8])
            assert_states_equal(e.store_state(), o.state(), G, P, L, ctx)


@pytest.mark.parametrize("P", rc.TICK_P)
def test_tick_full_mode_gpu(P):
    """Every group count, fuzz and snapshot-heavy states, every group its own mask."""
    for i, G in enumerate(rc.TICK_G):
        run_tick(P, G, seed=i, kind="snap" if i % 2 else "fuzz", export=bool(i % 3 == 0))


@pytest.mark.parametrize("mode", [TICK_LIGHT, TICK_AUTO])
@pytest.mark.parametrize("P", (2, 3, 5, 8))
def test_tick_light_and_auto_gpu(P, mode):
    for G, kind in ((9, "fuzz"), (33, "synth"), (65, "synth"), (65, "snap")):
        run_tick(P, G, seed=2, kind=kind, mode=mode, ticks=3)


@pytest.mark.parametrize("shards", (2, 3))
@pytest.mark.parametrize("mode", [TICK_FULL, TICK_LIGHT])
def test_tick_shards_gpu(mode, shards):
    """The mask pointer follows the shard's first group."""
    for P, G in ((3, 65), (5, 33), (8, 9)):
        run_tick(P, G, seed=3, kind="synth" if mode == TICK_LIGHT else "fuzz", mode=mode, shards=shards,
                 export=True)


def test_tick_device_buffers_gpu():
    run_tick(5, 65, seed=4, kind="fuzz", device=True)


def test_tick_chunk_edge_pass_origin_gpu():
    """Delivered followers merge across 256-entry chunk edges while the one cut
    off would have started the pass lower."""
    G, P, L, st, lp, reach = rc.chunk_edge_case()
    for mode in (TICK_FULL, TICK_LIGHT):
        o = Oracle(G, P, L, st)
        with Engine(G, P, L) as e:
            e.load_state(st)
            e.set_tick_mode(mode)
            e.set_reachable(reach)
            for k in range(2):
                want = masked_tick(o, lp, reach)
                assert np.array_equal(e.replicate_tick(lp), want)
                assert_states_equal(e.store_state(), o.state(), G, P, L, f"chunk edge, mode {mode}, tick {k}")
            cut = np.array([2 if g % 2 == 0 else 1 for g in range(G)])
            assert np.array_equal(o.state()["last_index"][np.arange(G) * P + cut], np.full(G, 39))


@pytest.mark.parametrize("mode", [TICK_FULL, TICK_LIGHT])
def test_start_and_tick_gpu(mode):
    """Start is local: the leader appends whatever the mask says."""
    P, G = 5, 65
    st, lp, reach, _ = rc.tick_case(P, G, 5, "synth")
    L = rc.TICK_L
    counts = ((np.arange(G) * 7) % 4).astype(np.int32)
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.set_tick_mode(mode)
        e.set_reachable(reach)
        for k in range(2):
            ok = (lp >= 0) & (lp < P) & (counts > 0)
            slots = (np.arange(G) * P + np.clip(lp, 0, P - 1))[ok].astype(np.int32)
            wi, wt, wl, werr = o.start(slots, counts[ok])
            want = masked_tick(o, lp, reach)
            got, (oi, ot, ol, err) = e.start_and_tick(lp, counts)
            assert np.array_equal(oi[ok], wi) and np.array_equal(ot[ok], wt) and np.array_equal(ol[ok], wl)
            assert np.array_equal(err[ok], werr)
            assert np.array_equal(got, want), (mode, k)
            assert_states_equal(e.store_state(), o.state(), G, P, L, f"start_and_tick mode {mode} tick {k}")


def test_set_clear_tick_and_count_gpu():
    """Set -> clear (NULL) -> the tick is the oracle's plain tick; the word count
    is refused while a mask is set and answers again after."""
    P, G = 5, 33
    st, lp, reach, _ = rc.tick_case(P, G, 6, "fuzz")
    L = rc.TICK_L
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.set_reachable(reach)
        out = np.zeros(3, np.int64)
        assert _abi.lib().mraft_replicate_tick_count(e._h, ptr(lp), ptr(out), HOST) == _abi.E_INVAL
        e.set_reachable(None)
        assert e.replicate_tick_count(lp) == o.replicate_tick_count(lp)
        assert np.array_equal(e.replicate_tick(lp), o.replicate_tick(lp))
        assert_states_equal(e.store_state(), o.state(), G, P, L, "set, clear, tick")


def test_light_fallback_count_gpu():
    """Light mode under a mask: the groups sent to the full tick are the settle
    rule's among the fully connected groups (what a plain light tick of those
    groups alone sends on) plus every running group with an incomplete mask."""
    P, G = 5, 65
    st, lp, reach, _ = rc.tick_case(P, G, 7, "synth")
    L = rc.TICK_L
    rec = {}
    masked_tick(Oracle(G, P, L, st), lp, full_mask(G, P), rec)
    incomplete = (reach & ((1 << P) - 1)) != (1 << P) - 1
    assert int((incomplete & rec["run"]).sum()) > 0 and int((~incomplete & rec["run"]).sum()) > 0
    with Engine(G, P, L) as plain:
        plain.load_state(st)
        plain.set_tick_mode(TICK_LIGHT)
        plain.replicate_tick(np.where(incomplete, -1, lp).astype(np.int32))
        plain.synchronize()
        settle_rule = plain.tick_light_fallbacks()
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.set_tick_mode(TICK_LIGHT)
        e.set_reachable(reach)
        want = masked_tick(o, lp, reach)
        assert np.array_equal(e.replicate_tick(lp), want)
        e.synchronize()
        assert e.tick_light_fallbacks() == settle_rule + int((incomplete & rec["run"]).sum())
        assert_states_equal(e.store_state(), o.state(), G, P, L, "light fallbacks")


# ---- the election round ----------------------------------------------------------------------------
def run_round(case, reach, R=None, null_flags=False, ctx=""):
    G, P, L = case["G"], case["P"], case["L"]
    mask = case["mask"] if R is None else case["mask"][:R]
    o = Oracle(G, P, L, case["st"])
    with Engine(G, P, L) as e:
        e.load_state(case["st"])
        e.set_reachable(reach)
        want = masked_election_rounds(o, mask, reach)
        if null_flags:
            assert _abi.lib().mraft_election_rounds(e._h, ptr(mask), len(mask), None, HOST) == 0
        else:
            assert np.array_equal(e.election_rounds(mask), want), ctx
        ec.assert_images_equal(e.store_state(), o.state(), G, P, L, ctx)
        assert np.array_equal(e.collect_persist(), o.collect_persist()), (ctx, "persist bits")


@pytest.mark.parametrize("P", (1, 2))
def test_round_exhaustive_every_mask_gpu(P):
    case = ec.exhaustive(P)
    for m in range(1 << P):
        run_round(case, np.full(case["G"], m | (0xF0 if m % 2 else 0), np.uint8), ctx=f"exhaustive P {P} mask {m}")


@pytest.mark.parametrize("m", range(8))
def test_round_p3_every_mask_gpu(m):
    """rc.P3_SAMPLE = 32,768 seeded groups of the exhaustive P = 3 set per mask."""
    case = rc.p3_sample(m)
    run_round(case, np.full(case["G"], m, np.uint8), ctx=f"P 3 mask {m}")


@pytest.mark.parametrize("P", ec.DIRECTED_P)
def test_round_directed_masks_gpu(P):
    case = ec.directed(P)
    runs = [(c, 0) for c in rc.ROUND_CLASSES] + [("voter_cut", k) for k in range(P - 1)]
    for i, (cls, k) in enumerate(runs):
        run_round(case, rc.directed_round_masks(case, cls, k), R=1 + i % 3, null_flags=(i == 2),
                  ctx=f"directed P {P} {cls} {k}")


def test_round_one_launch_equals_launch_per_round_gpu():
    case = rc.p3_sample(5)
    G, P, L, mask = case["G"], case["P"], case["L"], case["mask"]
    reach = np.random.default_rng(0x0E1).integers(0, 8, G).astype(np.uint8)
    for R in (1, 2, 3):
        with Engine(G, P, L) as a, Engine(G, P, L) as b:
            for x in (a, b):
                x.load_state(case["st"])
                x.set_reachable(reach)
            gfa = a.election_rounds(mask[:R])
            gfb = np.zeros(G, np.int32)
            for r in range(R):
                gfb |= b.election_rounds(mask[r:r + 1])
            assert np.array_equal(gfa, gfb)
            ec.assert_images_equal(a.store_state(), b.store_state(), G, P, L, f"R {R}")
            assert np.array_equal(a.collect_persist(), b.collect_persist())


# ---- the clock step ----------------------------------------------------------------------------------
def compare_step(e, m, now, send_all, ctx):
    G, P, L = m.G, m.P, m.L
    want = m.clock_step(now, send_all)
    got = e.clock_step(now, send_all)
    for n in CLOCK_OUTS:
        assert np.array_equal(got[n], want[n]), (ctx, n, np.nonzero(got[n] != want[n])[0][:8])
    assert_states_equal(e.store_state(), m.state(), G, P, L, ctx)
    for name, a, b in zip(("election_due", "heartbeat_due"), e.timers_store(), (m.ed, m.hd)):
        assert np.array_equal(a, b), (ctx, name, np.nonzero(a != b)[0][:8])
    return want


@pytest.mark.parametrize("P,G,send_all", CLOCK_CASES)
def test_clock_cases_with_changing_masks_gpu(P, G, send_all):
    L, st, ed, hd, m = rc.clock_model(P, G, send_all)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
        e.timers_load(ed, hd)
        if G >= 33:
            e.set_tick_mode((TICK_FULL, TICK_LIGHT, TICK_AUTO)[P % 3])
        for k in range(rc.CLOCK_STEPS):
            if k % rc.CLOCK_MASK_EVERY == 0:
                reach = rc.clock_masks(P, G, send_all, k // rc.CLOCK_MASK_EVERY)
                e.set_reachable(reach)
                m.set_reachable(reach)
            compare_step(e, m, NOW0 + k, send_all, f"clock P {P} G {G} send_all {send_all} step {k}")


# ---- the reference's scenarios on the co-resident path ------------------------------------------------
@pytest.mark.parametrize("P", (3, 5))
def test_reference_scenarios_gpu(P):
    """TestReElection2A, TestFailAgree2B, TestRejoin2B (P = 3) and
    TestFailNoAgree2B (P = 5) (src/raft/test_test.go), one per group, each
    group's schedule shifted by its index, on 64 groups: engine and model in
    lockstep, driven by set_reachable, start, clock_step and the compacted
    applier only."""
    G, L = 64, rc.SCEN_L
    cfg, W = rc.SCEN_CFG, rc.SCEN_PHASE
    names = rc.scenario_groups(P, G)
    shift = np.arange(G) % cfg["lo"]
    m = ReachModel(G, P, L)
    m.enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], 0)
    full = (1 << P) - 1
    reach = np.full(G, full, np.uint8)
    marked = np.zeros(G, np.int64)
    phase = np.full(G, -1)
    leader_of_term = [dict() for _ in range(G)]
    applied = [dict() for _ in range(G)]        # group -> Index -> term
    phase_commit = None
    n_phase = max(len(s[1]) for s in rc.SCENARIOS.values())
    phase_term = np.zeros((G, P), np.int64)
    checks = dict(majority_leader=0, no_quorum=0, agree=0, cut_leader_sends=0, two_leaders=0, rejoin_step_down=0,
                  cut_terms_rise=0)
    with Engine(G, P, L) as e:
        e.timers_enable(cfg["seed"], cfg["heartbeat"], cfg["lo"], cfg["hi"], 0)
        for t in range(1, n_phase * W + int(shift.max()) + 1):
            stt = m.state()
            role, term = stt["state"].reshape(G, P), stt["current_term"].reshape(G, P)
            conn = connected(reach, G, P)
            for g in range(G):
                sched = rc.SCENARIOS[names[g]][1]
                k = (t - 1 - shift[g]) // W
                if k == phase[g] or k < 0:
                    continue
                # the phase that ends: its conditions
                if phase[g] >= 0:
                    nconn = int(conn[g].sum())
                    lead = [p for p in range(P) if role[g, p] == LEADER and conn[g, p]]
                    if nconn > P // 2:
                        assert lead, (names[g], g, "no Leader among a connected majority", phase[g], t)
                        checks["majority_leader"] += 1
                    else:
                        # (a connected follower may still catch up to the commitIndex its
                        # leader already had: the group's highest commitIndex is what stands)
                        assert stt["commit_index"].reshape(G, P)[g].max() == phase_commit[g].max(), \
                            (names[g], g, "commit advanced without a majority")
                        checks["no_quorum"] += 1
                        # replicas cut off keep timing out: their terms rise, and nobody leads them
                        checks["cut_terms_rise"] += int((term[g] > phase_term[g])[~conn[g]].any())
                phase[g] = k
                if k < len(sched):
                    fn, mark = sched[k]
                    Lg = rc.visible_leader(role[g], term[g], conn[g])
                    if mark:
                        marked[g] = Lg
                    reach[g] = fn(P, Lg, int(marked[g]))
                else:
                    reach[g] = full
                if phase_commit is None:
                    phase_commit = stt["commit_index"].reshape(G, P).copy()
                phase_commit[g] = stt["commit_index"].reshape(G, P)[g]
                phase_term[g] = term[g]
            e.set_reachable(reach)
            m.set_reachable(reach)
            if t % 4 == 0:                        # Start at every Leader, the cut-off ones too
                slots = np.nonzero(stt["state"] == LEADER)[0].astype(np.int32)
                if len(slots):
                    a, b = e.start(slots, np.ones(len(slots), np.int32)), m.o.start(slots, np.ones(len(slots), np.int32))
                    for x, y in zip(a, b):
                        assert np.array_equal(x, y), (t, "start")
            conn = connected(reach, G, P)
            before = m.state()["state"].reshape(G, P).copy()
            want = compare_step(e, m, t, True, f"scenario P {P} tick {t}")
            stt = m.state()
            role, term = stt["state"].reshape(G, P), stt["current_term"].reshape(G, P)
            # at most one Leader per term; none elected without a connected majority
            for g, p in zip(*np.nonzero(role == LEADER)):
                assert leader_of_term[g].setdefault(int(term[g, p]), int(p)) == p, (g, "two Leaders in one term")
            lpo = want["leader_peer"]
            checks["cut_leader_sends"] += int(((lpo >= 0) & ~conn[np.arange(G), np.maximum(lpo, 0)]).sum())
            checks["two_leaders"] += int(((role == LEADER).sum(axis=1) >= 2).sum())
            checks["rejoin_step_down"] += int(((before == LEADER) & (role != LEADER) & conn).sum())
            new = (role == LEADER) & (before != LEADER)
            assert not (new & (conn.sum(axis=1) <= P // 2)[:, None]).any(), "a Leader elected without a majority"
            # the applier: engine and model agree, and every applied Index carries one term per group
            sl, fr, to, _ = e.collect_apply_compact()
            ofr, oto = m.o.collect_apply()
            has = oto >= ofr
            assert np.array_equal(sl, np.nonzero(has)[0]) and np.array_equal(fr, ofr[has]) and np.array_equal(to, oto[has])
            logs = logical_logs(stt, G, P, L)
            for s, a, b in zip(sl, fr, to):
                g = int(s) // P
                for i in range(int(a), int(b) + 1):
                    tm = int(logs[s, i - stt["dummy_index"][s]])
                    assert applied[g].setdefault(i, tm) == tm, (g, i, "two replicas applied different entries")
                    checks["agree"] += 1
    assert checks["majority_leader"] > G and checks["agree"] > G
    # a cut-off Leader that keeps sending, a second Leader beside it, the old one stepping
    # down once it is back
    # (TestFailNoAgree2B, the P = 5 schedule, never cuts its leader off)
    if P == 3:
        assert checks["cut_leader_sends"] > 0 and checks["two_leaders"] > 0 and checks["rejoin_step_down"] > 0, checks
    if P == 5 or "ReElection2A" in names:
        assert checks["no_quorum"] > 0 and checks["cut_terms_rise"] > 0, checks
