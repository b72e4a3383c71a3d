"""Every batched call of multiraft_amd/_calls.py three ways on one small
shape: where=DEVICE on device buffers, where=HOST on a twin engine, and the
CPU oracle. The outputs agree byte for byte, in the allocated form and in the
`out=` form (buffers prefilled with -1), and the three states are equal at
the end. The kernels themselves are covered elsewhere; this is about the
marshalling."""
import numpy as np
import pytest

from message_cases import all_follower_items, results_of
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import DEVICE, Engine, synth_seed, synth_tick_state
from multiraft_amd._abi import IS_ARGS, IS_RESULT, LEADER, RV_ARGS, RV_RESULT, from_words, to_words

pytestmark = pytest.mark.gpu

G, P, L = 8, 3, 32


class Trio:
    """The host engine, the device engine and the oracle, called alike."""

    def __init__(self, eh, ed, o):
        import torch
        self.torch, self.eh, self.ed, self.o = torch, eh, ed, o

    def dev(self, a):
        if a is None:
            return None
        return to_words(a, "cuda") if a.dtype.fields else self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def same(self, h, d, w, ctx):
        self.ed.synchronize()
        assert len(h) == len(d) == len(w), ctx
        for j, (a, t, b) in enumerate(zip(h, d, w)):
            if a is None:
                assert t is None and b is None, (ctx, j)
                continue
            assert b is ... or (a.dtype == b.dtype and a.tobytes() == b.tobytes()), (ctx, j, "host engine vs oracle")
            assert from_words(t, a.dtype).tobytes() == a.tobytes(), (ctx, j, "device vs host")

    def check(self, ctx, f, ins=(), f_oracle=None, device_allocates=True):
        """f(engine, inputs, **kw) -> the call's outputs in C order. Called
        once in the allocated form and once with out= on all three (the
        oracle through f_oracle, without out=, where it has no such call).
        Returns the host engine's first outputs."""
        torch = self.torch
        dins = [self.dev(a) for a in ins]
        h, w = f(self.eh, ins), (f_oracle or f)(self.o, ins)
        blank = lambda r: tuple(None if a is None else np.full_like(a, -1) for a in r)  # noqa: E731

        def blank_dev():
            out = tuple(None if a is None else
                        torch.full((len(a), a.dtype.itemsize // 4) if a.dtype.fields else (len(a),), -1,
                                   dtype=torch.int32, device="cuda") for a in h)
            torch.cuda.synchronize()               # the fills ran on torch's stream, the engines have their own
            return out
        if device_allocates:
            self.same(h, f(self.ed, dins, where=DEVICE), w, ctx + ", allocated")
        else:
            with pytest.raises(ValueError):        # no input to take the device from: out= both times
                f(self.ed, dins, where=DEVICE)
            do = blank_dev()
            f(self.ed, dins, where=DEVICE, out=do)
            self.same(h, do, w, ctx + ", allocated on the host side")
        ho, wo, do = blank(h), blank(h), blank_dev()
        f(self.eh, ins, out=ho)
        f(self.ed, dins, where=DEVICE, out=do)
        if f_oracle:
            wo = f_oracle(self.o, ins)
        else:
            f(self.o, ins, out=wo)
        self.same(ho, do, wo, ctx + ", out=")
        return h


def test_device_host_and_oracle_agree_gpu():
    st, lp, _ = synth_tick_state(G, P, L, seed=synth_seed(3))
    slots, peers = all_follower_items(lp, G, P)
    seg = np.concatenate([[0], np.cumsum(np.bincount(slots // P, minlength=G)[lp >= 0])]).astype(np.int64)
    leaders = (np.arange(G) * P + lp)[lp >= 0].astype(np.int32)
    o = Oracle(G, P, L, st)
    with Engine(G, P, L) as eh, Engine(G, P, L) as ed:
        eh.load_state(st)
        ed.load_state(st)
        t = Trio(eh, ed, o)
        # ---- AppendEntries: gather -> handle -> fold, Start, the applier
        args, gerr = t.check("gather_append_args", lambda e, i, **kw: e.gather_append_args(*i, **kw), (slots, peers))
        ok = gerr == 0
        assert ok.any()

        def handle(e, i, **kw):
            rep, err, res = e.handle_append_entries(i[0], None, results=True, **kw)
            return rep, res, err

        def handle_oracle(e, i):                   # no reply records on the oracle: `...` is not compared
            rep, err = e.handle_append_entries(i[0], None)
            return rep, ..., err
        rep, _, herr = t.check("handle_append_entries", handle, (args[ok],), f_oracle=handle_oracle)
        items, iseg = results_of(slots[ok], peers[ok], args[ok], rep, herr, G, P)
        flags, _ = t.check("process_append_replies", lambda e, i, **kw: e.process_append_replies(*i, **kw), (items, iseg))
        assert flags.any()
        counts = (1 + np.arange(len(leaders)) % 3).astype(np.int32)
        _, _, isl, _ = t.check("start", lambda e, i, **kw: e.start(*i, **kw), (leaders, counts))
        assert isl.any()
        t.check("collect_apply", lambda e, i, out=None, **kw:
                e.collect_apply(out=None if out is None else (*out, None, None), **kw), device_allocates=False)
        t.check("collect_apply(snapshots)", lambda e, i, **kw: e.collect_apply(True, **kw), device_allocates=False)
        # ---- snapshots: Snapshot at the leaders' commitIndex, gather -> handle -> fold
        sst = eh.store_state()
        t.check("snapshot", lambda e, i, **kw: (e.snapshot(*i, **kw),), (leaders, sst["commit_index"][leaders]))
        t.check("gather_install_snapshot_args", lambda e, i, **kw: e.gather_install_snapshot_args(*i, **kw),
                (slots, peers))
        sst = eh.store_state()
        ia = np.zeros(len(slots), IS_ARGS)
        ia["slot"], ia["term"], ia["leader_id"] = (slots // P) * P + peers, sst["current_term"][slots], slots % P
        ia["last_included_index"] = sst["dummy_index"][slots]
        ia["last_included_term"] = sst["log_term"][slots.astype(np.int64) * L + sst["log_head"][slots]]
        irep, ifl, ierr = t.check("handle_install_snapshot", lambda e, i, **kw: e.handle_install_snapshot(*i, **kw), (ia,))
        assert not ierr.any()
        ir = np.zeros(len(slots), IS_RESULT)
        ir["slot"], ir["peer"], ir["args_term"] = slots, peers, ia["term"]
        ir["args_last_included_index"], ir["reply_term"] = ia["last_included_index"], irep["term"]
        t.check("process_install_snapshot_replies",
                lambda e, i, **kw: e.process_install_snapshot_replies(*i, **kw), (ir, seg))
        # ---- elections: the first non-leader of every group stands
        cp = (st["state"].reshape(G, P) != LEADER).argmax(axis=1)
        cs = (np.arange(G) * P + cp).astype(np.int32)
        ra, serr = t.check("start_election", lambda e, i, **kw: e.start_election(*i, **kw), (cs,))
        assert not serr.any()
        q, src = np.tile(np.arange(P - 1), G), np.repeat(np.arange(G), P - 1)
        vp = np.where(q < cs[src] % P, q, q + 1)
        va = np.zeros(len(src), RV_ARGS)
        va["slot"], va["candidate_id"] = (cs[src] // P) * P + vp, cs[src] % P
        for f in ("term", "last_log_index", "last_log_term"):
            va[f] = ra[f][src]
        vrep, _ = t.check("handle_request_vote", lambda e, i, **kw: e.handle_request_vote(*i, **kw), (va,))
        vr = np.zeros(len(src), RV_RESULT)
        vr["slot"], vr["peer"], vr["args_term"] = cs[src], vp, va["term"]
        vr["reply_term"], vr["vote_granted"] = vrep["term"], vrep["vote_granted"]
        t.check("process_vote_replies", lambda e, i, **kw: e.process_vote_replies(*i, **kw),
                (vr, np.arange(G + 1, dtype=np.int64) * (P - 1)))
        # ---- GetState and persistence
        t.check("export_group_status", lambda e, i, **kw: e.export_group_status(*i, **kw), (lp,))
        t.check("collect_persist", lambda e, i, **kw: (e.collect_persist(**kw),), device_allocates=False)
        every = np.arange(G * P, dtype=np.int32)
        saved = [e.read_persistent(every) for e in (eh, ed, o)]       # host arrays only
        for hdr, terms in saved[1:]:
            assert np.array_equal(hdr, saved[0][0]) and np.array_equal(terms, saved[0][1])
        errs = [e.restore(*saved[0]) for e in (eh, ed, o)]
        assert not errs[0].any() and all(np.array_equal(x, errs[0]) for x in errs[1:])
        assert_states_equal(eh.store_state(), o.state(), G, P, L, "host engine vs oracle")
        assert_states_equal(ed.store_state(), o.state(), G, P, L, "device engine vs oracle")
