"""The timer calls with MRAFT_DEVICE buffers, and the header's promise that
with MRAFT_DEVICE a call only enqueues work (include/mraft.h "timers"; the
message path's counterpart is tests/test_handler_async.py): mraft_timers_load,
mraft_timers_arm, mraft_ticker (device lists and device int64 counts),
mraft_timers_note on device copies of records the message path produced, and
mraft_timers_store are enqueued behind a device spin with no host
synchronisation in between; then K back-to-back mraft_clock_step calls with
device outputs on two tick shards. The calls return while the stream is still
busy, and afterwards every buffer, the state and the timers equal the model
run with the same calls.

Shapes: G*P = 1,285 slots (six blocks of 256, the last partial) and 262,155
slots (1,025 blocks: the scan's second chunk of 1,024)."""
import ctypes

import numpy as np
import pytest

from gpu_support import behind_spin
from oracle_lib import assert_states_equal
from timers_cases import CFG, due_timers, leaders_in_place_state
from timers_model import TimersModel

from multiraft_amd import DEVICE, Engine, _abi
from multiraft_amd._abi import LEADER, NOTE_RV_FOLDED, NOTE_RV_HANDLED, RV_ARGS, RV_RESULT, to_words

pytestmark = pytest.mark.gpu

SHAPES = [(257, 5, 8), (52431, 5, 4)]
OUTS = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")
SPIN = int(2e8)  # ~0.1 s of device spin ahead of the calls


def on_device(a):
    """A device copy of a numpy array (records: their words)."""
    import torch
    return to_words(a, "cuda") if a.dtype.fields else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_timers(e, m, ctx):
    for name, a, b in zip(("election_due", "heartbeat_due"), e.timers_store(), (m.ed, m.hd)):
        bad = np.nonzero(a != b)[0][:8]
        assert not len(bad), f"{ctx}: {name} differs at {bad}: {a[bad]} vs {b[bad]}"


def vote_records(e, o, st, G, P):
    """One RequestVote round, one candidate per group, through the message path
    of the engine and of the oracle (host buffers, synchronous): the handled
    (args, replies, item_err) and the tallied (results, flags, item_err)."""
    cp = (st["state"].reshape(G, P) != LEADER).argmax(axis=1)       # the first non-leader
    cs = (np.arange(G) * P + cp).astype(np.int32)
    ra, serr = e.start_election(cs)
    ora, oserr = o.start_election(cs)
    assert np.array_equal(ra, ora) and not serr.any() and not oserr.any()
    q = np.tile(np.arange(P - 1), G)
    src = np.repeat(np.arange(G), P - 1)
    vp = np.where(q < cs[src] % P, q, q + 1)
    va = np.zeros(len(src), dtype=RV_ARGS)
    va["slot"], va["candidate_id"] = (cs[src] // P) * P + vp, cs[src] % P
    for f in ("term", "last_log_index", "last_log_term"):
        va[f] = ra[f][src]
    rep, herr = e.handle_request_vote(va)
    orep, oherr = o.handle_request_vote(va)
    assert np.array_equal(rep, orep) and np.array_equal(herr, oherr)
    res = np.zeros(len(src), dtype=RV_RESULT)
    res["slot"], res["peer"], res["args_term"] = cs[src], vp, va["term"]
    res["reply_term"], res["vote_granted"] = rep["term"], rep["vote_granted"]
    seg = np.arange(G + 1, dtype=np.int64) * (P - 1)
    tfl, terr = e.process_vote_replies(res, seg)
    otfl, oterr = o.process_vote_replies(res, seg)
    assert np.array_equal(tfl, otfl) and np.array_equal(terr, oterr)
    assert (rep["vote_granted"] != 0).any() and (rep["vote_granted"] == 0).any()
    assert (tfl & _abi.F_BECAME_LEADER).any()
    return (va, rep, herr), (res, tfl, terr)


@pytest.mark.parametrize("G,P,L", SHAPES)
def test_timer_calls_only_enqueue(G, P, L):
    import torch
    lib = _abi.lib()
    rng = np.random.default_rng(900 + G)
    gp = G * P
    st = leaders_in_place_state(G, P, L, rng, seed=900 + G)
    m = TimersModel(G, P, L, st)
    T = 500
    ed, hd = due_timers(rng, gp, T, 0.5), due_timers(rng, gp, T, 0.5)
    arm = np.concatenate([rng.integers(0, gp, size=gp // 7), [-1, gp, 0, 0]]).astype(np.int32)
    cap = gp // 8  # the first ticker call's lists are cut, the second takes the rest
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], 0)
        m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], 0)
        handled, tallied = vote_records(e, m.o, st, G, P)
        d_ed, d_hd, d_arm = on_device(ed), on_device(hd), on_device(arm)
        d_handled, d_tallied = [on_device(a) for a in handled], [on_device(a) for a in tallied]
        lists = [torch.full((gp,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
        counts = [torch.full((1,), -7, dtype=torch.int64, device="cuda") for _ in range(4)]
        o_ed, o_hd = (torch.zeros(gp, dtype=torch.int32, device="cuda") for _ in range(2))
        dst = _abi.MraftTimersSoa(o_ed.data_ptr(), o_hd.data_ptr())
        h = e._h
        # every call returns with the device still behind the spin: nothing waits on it
        with behind_spin(e, SPIN, "a timer call"):
            e.timers_load(d_ed, d_hd, where=DEVICE)
            e.timers_arm(d_arm, T - 10, where=DEVICE)
            for k, c in enumerate((cap, gp)):   # the ticker and the store: host wrappers only, so raw
                assert lib.mraft_ticker(h, T, lists[2 * k].data_ptr(), c, counts[2 * k].data_ptr(),
                                        lists[2 * k + 1].data_ptr(), c, counts[2 * k + 1].data_ptr(), DEVICE) == 0, \
                    _abi.last_error()
            for kind, (r, oc, ie) in ((NOTE_RV_HANDLED, d_handled), (NOTE_RV_FOLDED, d_tallied)):
                e.timers_note(kind, r, oc, ie, T + 1, where=DEVICE)
            assert lib.mraft_timers_store(h, ctypes.byref(dst), DEVICE) == 0, _abi.last_error()
        # the model, with the same calls
        m.load(ed, hd)
        m.arm(arm, T - 10)
        for k, c in enumerate((cap, gp)):
            we, wne, wh, wnh = m.ticker(T, c, c)
            assert (int(counts[2 * k].item()), int(counts[2 * k + 1].item())) == (wne, wnh), k
            ge, gh = lists[2 * k].cpu().numpy(), lists[2 * k + 1].cpu().numpy()
            assert np.array_equal(ge[:len(we)], we) and np.array_equal(gh[:len(wh)], wh), k
            assert (ge[len(we):] == -7).all() and (gh[len(wh):] == -7).all(), k  # nothing past the list
            if k == 0:
                assert wne > cap and wnh > 0 and len(we) == cap  # the cut was a real one
        m.note(NOTE_RV_HANDLED, *handled, T + 1)
        m.note(NOTE_RV_FOLDED, *tallied, T + 1)
        assert np.array_equal(o_ed.cpu().numpy(), m.ed) and np.array_equal(o_hd.cpu().numpy(), m.hd)
        same_timers(e, m, "after the enqueued calls")
        assert_states_equal(e.store_state(), m.state(), G, P, L, "timer calls leave the state alone")


@pytest.mark.parametrize("mode", [_abi.TICK_LIGHT, _abi.TICK_FULL], ids=["light", "full"])
@pytest.mark.parametrize("G,P,L", SHAPES)
def test_clock_steps_only_enqueue(G, P, L, mode):
    """K back-to-back clock steps, each with output buffers of its own, on two
    tick shards: A-C, the sharded tick and step E of one step are ordered on
    the device against the next step's, with no host wait anywhere."""
    import torch
    K, T = 4, 700
    rng = np.random.default_rng(950 + G)
    gp = G * P
    st = leaders_in_place_state(G, P, L, rng, seed=950 + G)
    m = TimersModel(G, P, L, st)
    ed, hd = due_timers(rng, gp, T, 1 / 3), due_timers(rng, gp, T, 1 / 3)
    with Engine(G, P, L) as e:
        e.load_state(st)
        e.set_tick_shards(2)
        e.set_tick_mode(mode)
        e.timers_enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], T)
        m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], T)
        e.timers_load(ed, hd)
        m.load(ed, hd)
        outs = [{n: torch.full((G,), 77, dtype=torch.uint8 if n == "cand_mask" else torch.int32, device="cuda")
                 for n in OUTS} for _ in range(K)]
        with behind_spin(e, SPIN, "a clock step"):
            for k in range(K):
                e.clock_step(T + k, bool(k % 2), where=DEVICE, out=outs[k])
        for k in range(K):
            want = m.clock_step(T + k, bool(k % 2))
            for n in OUTS:
                got = outs[k][n].cpu().numpy()
                assert np.array_equal(got, want[n]), (k, n, np.nonzero(got != want[n])[0][:8])
        same_timers(e, m, f"{K} clock steps")
        assert_states_equal(e.store_state(), m.state(), G, P, L, f"{K} clock steps, no host sync")
    assert m.stats["grants"] and m.stats["elected"]
