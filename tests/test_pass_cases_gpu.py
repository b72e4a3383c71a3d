"""The directed boundary matrix of the streaming merge pass
(tests/pass_cases.py, pinned against the oracle and against its own claimed
cells by tests/test_pass_cases.py) through the C ABI, bit for bit against the
C oracle: group flags, replies, item errors and the whole state.

Per family and form: mraft_replicate_tick under MRAFT_TICK_FULL with 1 and 2
shards, MRAFT_TICK_LIGHT (the built groups do not settle: k_tick_list, the
same body as another kernel) and MRAFT_TICK_AUTO, each followed by a second
tick on the resulting state (the followers have caught up: the "everything
matches" exits at the new positions); mraft_replicate_tick_count against the
oracle's count (the COUNT instantiation of the pass); the message path gather
-> HandleAppendEntries by reference and by value -> fold; the `bound` form's
states through mraft_bind_state with log_term 4, 8 and 12 B past a 16-B
boundary; family D's messages with MRAFT_AE_ENTRIES_SORTED forced on (a false
claim wherever the descent lies inside the message); and family V's buffer
layouts, from host buffers and from a device buffer bound off a 16-B boundary."""
import functools

import numpy as np
import pytest

import light_cases as lc
import pass_cases as pc
from message_cases import all_follower_items, external_entries, results_of
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import DEVICE, TICK_AUTO, TICK_FULL, TICK_LIGHT, Engine
from multiraft_amd._abi import AE_ENTRIES_SORTED, AE_REPLY, from_words, to_words

pytestmark = pytest.mark.gpu

CASES = [("M", f, 0) for f in ("vec", "mis1", "odd")] + [("W", f, 0) for f in pc.FORMS] + [("F", f, 0) for f in pc.FORMS] \
    + [("N", "vec", P) for P in pc.N_PEERS] + [("S", f, 0) for f in ("vec", "mis2", "odd")] \
    + [("C", "vec", 2), ("C", "vec", 5)] + [("D", f, 0) for f in pc.D_FORMS] + [("V", "vec", 0)]
IDS = [f"{a}-{b}" + (f"-P{p}" if p else "") for a, b, p in CASES]
MODES = [(TICK_FULL, 1), (TICK_FULL, 2), (TICK_LIGHT, 1), (TICK_AUTO, 1)]


@functools.lru_cache(maxsize=2)
def _oracle_ticks(key):
    """The oracle's two ticks on the case, computed once: per tick the group
    flags and the state after it; and the count of the first tick."""
    c = pc.case(*key)
    o = Oracle(c.G, c.P, c.L, c.state)
    count = o.replicate_tick_count(c.leader_peer)
    out = []
    for _ in range(2):
        gf = o.replicate_tick(c.leader_peer)
        out.append((gf, o.store_state()))
    return count, out


@pytest.mark.parametrize("mode,shards", MODES, ids=["full1", "full2", "light", "auto"])
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_tick_gpu(key, mode, shards):
    c = pc.case(*key)
    G, P, L, lp = c.G, c.P, c.L, c.leader_peer
    count, ticks = _oracle_ticks(key)
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        e.set_tick_shards(shards)
        e.set_tick_mode(mode)
        if (mode, shards) == (TICK_FULL, 1):
            assert e.replicate_tick_count(lp) == count, f"{c.name}: tick count"
        for k, (ogf, ost) in enumerate(ticks):
            ctx = f"{c.name} mode {mode} shards {shards} tick {k}"
            gf = e.replicate_tick(lp)
            bad = np.flatnonzero(gf != ogf)
            assert len(bad) == 0, f"{ctx}: group flags at {bad[:8]}: {[c.kinds[g] for g in bad[:8]]}"
            assert_states_equal(e.store_state(), ost, G, P, L, ctx)
            if mode == TICK_LIGHT and k == 0:
                # the path: the groups the light launch's stated rule does not settle ran the pass in k_tick_list
                e.synchronize()
                fb, listed = e.tick_light_fallbacks(), int(lc.settle_rule(c.state, P, L, lp, None).sum())
                print(f"LIGHTPATH {c.name} groups={G} listed={fb} rule={listed}")
                assert fb == listed > 0, f"{ctx}: {fb} groups listed, the rule says {listed}"


def _message_step(e, o, c, by, ctx):
    G, P, L = c.G, c.P, c.L
    slots, peers = all_follower_items(c.leader_peer, G, P)
    args, gerr = e.gather_append_args(slots, peers)
    oargs, ogerr = o.gather_append_args(slots, peers)
    assert np.array_equal(args, oargs) and np.array_equal(gerr, ogerr), f"{ctx}: gather"
    ok = gerr == 0
    if by == "value":
        ext, buf = external_entries(args, ok, o.state(), L, misalign=True)
        batch = ext[ok]
    else:
        batch, buf = args[ok], None
    rep, herr = e.handle_append_entries(batch, buf)
    orep, oherr = o.handle_append_entries(batch, buf)
    bad = np.flatnonzero((herr != oherr) | (rep != orep))
    assert len(bad) == 0, f"{ctx}: replies at items {bad[:8]}: {[c.kinds[int(batch['slot'][i]) // P] for i in bad[:8]]}"
    res, seg = results_of(slots[ok], peers[ok], args[ok], rep, herr, G, P)
    f, ferr = e.process_append_replies(res, seg)
    of, oferr = o.process_append_replies(res, seg)
    assert np.array_equal(f, of) and np.array_equal(ferr, oferr), f"{ctx}: fold"


@pytest.mark.parametrize("by", ["reference", "value"])
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_message_path_gpu(key, by):
    c = pc.case(*key)
    G, P, L = c.G, c.P, c.L
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        for step in range(2):   # the second step: every follower caught up
            ctx = f"{c.name} by {by} step {step}"
            _message_step(e, o, c, by, ctx)
            assert_states_equal(e.store_state(), o.state(), G, P, L, ctx)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("family", ["F", "W"])
def test_bound_form_gpu(family, off):
    """Rows aligned alike at L = 1024 with log_term bound `off` words past a
    16-B boundary: the tick and the by-reference handler take the dword
    forms. Two ticks, then a message step on the same engine."""
    import torch
    key = (family, "bound", 0)
    c = pc.case(*key)
    G, P, L, lp = c.G, c.P, c.L, c.leader_peer
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v.copy()).to(dev) for k, v in c.state.items()}
    n = len(c.state["log_term"])
    big = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    big[off:off + n] = d["log_term"]
    d["log_term"] = big[off:off + n]
    assert d["log_term"].data_ptr() % 16 == 4 * off
    torch.cuda.synchronize()   # the copies ran on torch's stream, the engine has its own
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L, alloc=False) as e:
        e.bind(d)
        for k in range(2):
            ctx = f"{c.name} log base +{off} words tick {k}"
            gf, ogf = e.replicate_tick(lp), o.replicate_tick(lp)
            bad = np.flatnonzero(gf != ogf)
            assert len(bad) == 0, f"{ctx}: group flags at {bad[:8]}: {[c.kinds[g] for g in bad[:8]]}"
            e.synchronize()
            assert_states_equal({k2: v.cpu().numpy() for k2, v in d.items()}, o.state(), G, P, L, ctx)
        ctx = f"{c.name} log base +{off} words, messages"
        _message_step(e, o, c, "reference", ctx)
        e.synchronize()
        assert_states_equal({k2: v.cpu().numpy() for k2, v in d.items()}, o.state(), G, P, L, ctx)


def test_bound_form_first_messages_gpu():
    """The by-reference handler on the bound states as built (every follower
    still behind): log_term 4 B past a 16-B boundary."""
    import torch
    c = pc.case("F", "bound", 0)
    G, P, L = c.G, c.P, c.L
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v.copy()).to(dev) for k, v in c.state.items()}
    n = len(c.state["log_term"])
    big = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    big[1:1 + n] = d["log_term"]
    d["log_term"] = big[1:1 + n]
    assert d["log_term"].data_ptr() % 16 == 4
    torch.cuda.synchronize()   # the copies ran on torch's stream, the engine has its own
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L, alloc=False) as e:
        e.bind(d)
        _message_step(e, o, c, "reference", c.name)
        e.synchronize()
        assert_states_equal({k: v.cpu().numpy() for k, v in d.items()}, o.state(), G, P, L, c.name)


@pytest.mark.parametrize("by", ["reference", "value"])
@pytest.mark.parametrize("form", pc.D_FORMS)
def test_descent_flag_forced_gpu(form, by):
    """Family D with MRAFT_AE_ENTRIES_SORTED set on every message, whatever
    the leader's proof says: the handler's own check of the shipped entries
    (DescTrack on the pass's loads) decides the follower's terms_sorted."""
    c = pc.case("D", form)
    G, P, L = c.G, c.P, c.L
    slots, peers = all_follower_items(c.leader_peer, G, P)
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        args, gerr = e.gather_append_args(slots, peers)
        oargs, ogerr = o.gather_append_args(slots, peers)
        assert np.array_equal(args, oargs) and not gerr.any() and not ogerr.any()
        args["flags"] |= AE_ENTRIES_SORTED
        buf = None
        if by == "value":
            args, buf = external_entries(args, gerr == 0, o.state(), L, misalign=True)
        rep, herr = e.handle_append_entries(args, buf)
        orep, oherr = o.handle_append_entries(args, buf)
        bad = np.flatnonzero((herr != oherr) | (rep != orep))
        assert len(bad) == 0, f"{c.name}: replies at {bad[:8]}: {[c.kinds[int(args['slot'][i]) // P] for i in bad[:8]]}"
        got = e.store_state()
    bad = np.flatnonzero(got["terms_sorted"] != o.state()["terms_sorted"])
    assert len(bad) == 0, f"{c.name} by {by}: terms_sorted at {bad[:8]}: {[c.kinds[s // P] for s in bad[:8]]}"
    assert_states_equal(got, o.state(), G, P, L, f"{c.name} forced flag by {by}")


def _value_batch(c, layout):
    G, P, L = c.G, c.P, c.L
    slots, peers = all_follower_items(c.leader_peer, G, P)
    o = Oracle(G, P, L, c.state)
    args, gerr = o.gather_append_args(slots, peers)
    ok = gerr == 0
    a2, buf, base_off = pc.value_layout(args, ok, o.state(), L, layout, eligible=pc.merging_items(c, slots, peers))
    return o, np.ascontiguousarray(a2[ok]), buf, base_off


@pytest.mark.parametrize("layout", ["residue", "lastword", "shared"])
def test_value_layouts_host_gpu(layout):
    """Family V from a host buffer (the engine's own 16-B aligned copy)."""
    c = pc.case("N", "vec", 5) if layout == "shared" else pc.case("V", "vec")
    o, batch, buf, base_off = _value_batch(c, layout)
    assert base_off == 0
    with Engine(c.G, c.P, c.L) as e:
        e.load_state(c.state)
        rep, herr = e.handle_append_entries(batch, buf)
        orep, oherr = o.handle_append_entries(batch, buf)
        bad = np.flatnonzero((herr != oherr) | (rep != orep))
        assert len(bad) == 0, f"{c.name} {layout}: replies at {bad[:8]}"
        assert_states_equal(e.store_state(), o.state(), c.G, c.P, c.L, f"{c.name} {layout}")


@pytest.mark.parametrize("layout", ["word0-1", "word0-2", "word0-3", "lastword", "residue"])
def test_value_layouts_device_gpu(layout):
    """Family V from a device buffer bound where the layout says: a message
    that begins at word 0 of a buffer 4, 8 or 12 B past a 16-B boundary (the
    dwordx4 group of its first entry would start before the buffer) and one
    that ends on the last word of a buffer whose end is short of a 16-B
    boundary: the dword form must be chosen for both."""
    import torch
    c = pc.case("V", "vec")
    G, P, L = c.G, c.P, c.L
    o, batch, buf, base_off = _value_batch(c, layout)
    n = len(batch)
    dev = torch.device("cuda", 0)
    big = torch.full((len(buf) + 8,), pc.POISON, dtype=torch.int32, device=dev)
    big[base_off:base_off + len(buf)] = torch.from_numpy(buf).to(dev)
    buf_d = big[base_off:base_off + len(buf)]
    assert buf_d.data_ptr() % 16 == 4 * base_off
    args_d = to_words(batch, dev)
    rep_d = torch.zeros((n, AE_REPLY.itemsize // 4), dtype=torch.int32, device=dev)
    err_d = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()   # the fills and copies ran on torch's stream, the engine has its own
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        e.handle_append_entries(args_d, buf_d, where=DEVICE, out=(rep_d, None, err_d))
        e.synchronize()
        rep, herr = from_words(rep_d, AE_REPLY), err_d.cpu().numpy()
        orep, oherr = o.handle_append_entries(batch, buf)
        bad = np.flatnonzero((herr != oherr) | (rep != orep))
        assert len(bad) == 0, f"{c.name} {layout}: replies at {bad[:8]}"
        assert_states_equal(e.store_state(), o.state(), G, P, L, f"{c.name} {layout}, device buffer")
