"""The engine's scratch ranges on the GPU: the by-reference AppendEntries
handler's buffers (one of them epoch-tagged and kept from call to call: the
ordered fallback's reader counts), the host-mode staging of the calls that
stage the most buffers, and the clock step's and the applier's own slots, all
on one engine, interleaved. No staged buffer may land on a buffer another call
still relies on: every call's outputs and the state after it equal the
oracle's, and the heavy batch is exact again after the staging calls."""
import numpy as np
import pytest

from message_cases import deferred_graph_batch, deferred_graph_state
from oracle_lib import Oracle, assert_states_equal
from timers_model import TimersModel

from multiraft_amd import Engine, synth_tick_state

pytestmark = pytest.mark.gpu

CFG = dict(seed=11, heartbeat=3, lo=5, hi=12)
CLOCK_OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")


# stage capacity 0: every staged item takes the ordered fallback (the
# epoch-tagged buffer is in use); the default: the staged path
@pytest.mark.parametrize("cap", [0, None])
def test_scratch_ranges_interleaved_gpu(cap):
    G, P, L = 64, 5, 64
    rng = np.random.default_rng(705)
    st, c = deferred_graph_state(G, P, L, rng)
    heavy = deferred_graph_batch(st, G, P, L, c, rng, G * P)
    o = Oracle(G, P, L, st)
    orep, oerr = o.handle_append_entries(heavy, None)
    want = o.state()
    assert (oerr == 0).sum() > G * P // 2
    st2, lp, _ = synth_tick_state(G, P, L, seed=706)
    m = TimersModel(G, P, L, st2)       # m.o: the oracle of the staging calls
    m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], 0)
    counts = rng.integers(0, 4, size=G).astype(np.int32)

    def heavy_call(e, ctx):
        e.load_state(st)
        rep, err = e.handle_append_entries(heavy, None)
        assert np.array_equal(err, oerr) and np.array_equal(rep, orep), ctx
        assert_states_equal(e.store_state(), want, G, P, L, ctx)

    with Engine(G, P, L) as e:
        if cap is not None:
            e.set_stage_capacity(cap)
        heavy_call(e, "heavy batch")
        e.load_state(st2)
        # mraft_start_and_tick: seven staged buffers
        gf, outs = e.start_and_tick(lp, counts)
        idx, term = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
        isl, err = np.zeros(G, np.int32), np.zeros(G, np.int32)
        sel = np.flatnonzero(counts != 0)
        idx[sel], term[sel], isl[sel], err[sel] = m.o.start((sel * P + lp[sel]).astype(np.int32), counts[sel])
        for a, b, name in zip(outs, (idx, term, isl, err), ("index", "term", "is_leader", "err")):
            assert np.array_equal(a, b), name
        assert np.array_equal(gf, m.o.replicate_tick(lp))
        assert_states_equal(e.store_state(), m.state(), G, P, L, "start_and_tick")
        # mraft_collect_apply_compact with the snapshot outputs: six
        ofr, oto, osi, ost = m.o.collect_apply(snapshots=True)
        listed = np.nonzero((oto >= ofr) | (osi >= 0))[0]
        sl, si, stm, fr, to, n = e.collect_apply_compact(snapshots=True)
        assert n == len(listed) > 0 and np.array_equal(sl, listed)
        assert np.array_equal(fr, ofr[listed]) and np.array_equal(to, oto[listed])
        assert np.array_equal(si, osi[listed]) and np.array_equal(stm, ost[listed])
        assert_states_equal(e.store_state(), m.state(), G, P, L, "collect_apply_compact")
        # mraft_clock_step with every output: six, heartbeats and elections due
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], 0)
        for now in (4, 9):
            got, exp = e.clock_step(now), m.clock_step(now)
            for name in CLOCK_OUTS:
                assert np.array_equal(got[name], exp[name]), (now, name)
            ed, hd = e.timers_store()
            assert np.array_equal(ed, m.ed) and np.array_equal(hd, m.hd), now
            assert_states_equal(e.store_state(), m.state(), G, P, L, f"clock_step {now}")
        assert m.stats["grants"] > 0 and (exp["leader_peer"] >= 0).any()
        heavy_call(e, "heavy batch after the staging calls")
