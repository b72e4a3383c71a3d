"""Directed cases for the light tick's launch (k_tick_lite, MRAFT_TICK_LIGHT in
include/mraft.h). A group ends in the same state whether the light launch
settles it or lists it for the full tick, so a bit-exact comparison with the
oracle proves the light launch's code only where the group really settled
there. The states here (tests/light_cases.py, pinned against the oracle by
tests/test_light_cases.py) are built group by group, each tagged light or
listed by the stated settle rule, and every case asserts the path as well as
the result: mraft_tick_light_fallbacks equals the number of listed tags, and
0 in the variant that holds a family's light-tagged groups only.

Per case, P = 2..8, capacity 37 / 64 / 99 / 256 and 1 or 3 shards: one tick
(mraft_replicate_tick_export, or mraft_start_and_tick where the case fuses
Start) compared with the oracle's Start (raft.go:90-104) and tick
(raft_append_entry.go:20-162) bit for bit (group flags, the GetState words,
Start's outputs, the whole state with its persist bits), the path, then two
more ticks with Start of 0-3 entries compared the same way, where a wrong
nextIndex or terms_sorted word left by the first tick shows.

Also: families B and C (fused Start) under MRAFT_TICK_AUTO and
MRAFT_TICK_FULL; engines of 1 .. 255 groups (partial waves and workgroups,
fewer than eight workgroups, list regions filled exactly); and the
negative-count rule of mraft_start_and_tick."""
import numpy as np
import pytest

import light_cases as lc
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import TICK_AUTO, TICK_FULL, TICK_LIGHT, Engine
from multiraft_amd._abi import ITEM_BAD_SLOT

pytestmark = pytest.mark.gpu

START_NAMES = ("index", "term", "is_leader", "err")


def _tick(e, o, lp, counts, G, P, L, ctx):
    """One tick on both sides, everything compared. counts None: Start is not
    part of the tick. Returns Start's outputs (None without Start)."""
    outs = None
    if counts is None:
        gf, cm, tl = e.replicate_tick_export(lp)
        ogf = o.replicate_tick(lp)
    else:
        gf, outs = e.start_and_tick(lp, counts)
        ogf, oouts = lc.oracle_start_and_tick(o, lp, counts, G, P)
        for a, b, name in zip(outs, oouts, START_NAMES):
            assert np.array_equal(a, b), f"{ctx}: Start {name} at {np.flatnonzero(a != b)[:8]}"
        cm, tl = e.export_group_status(lp)
    assert np.array_equal(gf, ogf), f"{ctx}: group flags at {np.flatnonzero(gf != ogf)[:8]}"
    oc, otl = o.export_group_status(lp)
    assert np.array_equal(cm, oc) and np.array_equal(tl, otl), f"{ctx}: export words"
    assert_states_equal(e.store_state(), o.state(), G, P, L, ctx)
    return outs


def _run(c, shards, mode, path, follow=2):
    G, P, L, lp = c.G, c.P, c.L, c.leader_peer
    ctx = f"{c.name} P={P} L={L} shards={shards} mode={mode}"
    rng = np.random.default_rng(1000 * L + 10 * P + shards)
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        e.set_tick_shards(min(shards, G))
        e.set_tick_mode(mode)
        outs = _tick(e, o, lp, c.counts, G, P, L, ctx + " tick 0")
        if outs is not None:  # ... and what the case intends, errors included
            for a, b, name in zip(outs, c.start_expect, START_NAMES):
                assert np.array_equal(a, b), f"{ctx}: intended Start {name}"
        if path:
            e.synchronize()
            fb = e.tick_light_fallbacks()
            print(f"LIGHTPATH {c.name} P={P} L={L} shards={shards} groups={G} light={G - fb} listed={fb}")
            assert fb == c.n_listed, f"{ctx}: {fb} groups listed, {c.n_listed} tagged"
        for k in range(follow):
            cnt = rng.integers(0, 4, size=G).astype(np.int32)
            if c.counts is None:  # Start as its own call between the ticks
                sel = np.flatnonzero((cnt > 0) & (lp >= 0) & (lp < P))
                slots = (sel * P + lp[sel]).astype(np.int32)
                for a, b, name in zip(e.start(slots, cnt[sel]), o.start(slots, cnt[sel]), START_NAMES):
                    assert np.array_equal(a, b), f"{ctx}: follow-up Start {name}"
                _tick(e, o, lp, None, G, P, L, f"{ctx} tick {k + 1}")
            else:
                _tick(e, o, lp, cnt, G, P, L, f"{ctx} tick {k + 1}")


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("L", lc.CAPACITIES)
@pytest.mark.parametrize("P", lc.PEERS)
@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_directed_case_gpu(name, P, L, shards):
    """The result against the oracle and the path: exactly the listed-tagged
    groups go to the full tick, none in a `-light` case."""
    c = lc.case(name, P, L)
    if name.endswith("-light"):
        assert c.n_listed == 0
    _run(c, shards, TICK_LIGHT, path=True)


@pytest.mark.parametrize("mode", [TICK_AUTO, TICK_FULL])
@pytest.mark.parametrize("P", lc.PEERS)
@pytest.mark.parametrize("name", [n for n in lc.CASE_NAMES if n[0] in "BC"])
def test_fused_start_auto_full_gpu(name, P, mode):
    """mraft_start_and_tick on the fused-Start families under MRAFT_TICK_AUTO
    (Start inside the light launch while AUTO chooses it) and MRAFT_TICK_FULL
    (Start as its own launch): the result only."""
    for L in lc.CAPACITIES:
        _run(lc.case(name, P, L), 1 + P % 2, mode, path=False)


@pytest.mark.parametrize("P", [2, 5, 8])
@pytest.mark.parametrize("G", [1, 7, 9, 31, 33, 255])
def test_tiny_engines_gpu(G, P):
    """1 .. 255 groups, every one settling in the light launch and every one
    listed (appends of 65 entries): partial waves (G < 8), partial workgroups
    (G not a multiple of 32), fewer than eight workgroups in the launch's XCD
    remap, and, with all listed, every XCD's list region filled to its
    capacity."""
    light, listed = lc.tiny_cases(G, P)
    for shards in sorted({1, min(3, G)}):
        _run(light, shards, TICK_LIGHT, path=True)
        _run(listed, shards, TICK_LIGHT, path=True)


@pytest.mark.parametrize("L", [37, 64])
@pytest.mark.parametrize("P", [2, 5])
@pytest.mark.parametrize("name", ["B-mixed", "C-mixed", "C-top-light", "bad-slot"])
def test_directed_start_items_gpu(name, P, L):
    """The directed Start cases through the item-level mraft_start (k_start),
    which shares Start's rule with mraft_start_and_tick's two kernels: the
    groups oracle_start_and_tick selects (leader_peer in range, counts != 0)
    as one call of slots and counts, against the case's intended outputs
    (both sides of the ring's capacity and of the Index domain, negative
    counts), the oracle's Start, and the whole state."""
    c = lc.bad_slot_case(P, L) if name == "bad-slot" else lc.case(name, P, L)
    G, lp = c.G, c.leader_peer
    ctx = f"{name} P={P} L={L} mraft_start"
    sel = np.flatnonzero((lp >= 0) & (lp < P) & (c.counts != 0))
    assert len(sel)
    slots, cnt = (sel * P + lp[sel]).astype(np.int32), c.counts[sel].astype(np.int32)
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        outs = e.start(slots, cnt)
        oouts = o.start(slots, cnt)
        for a, want, b, nm in zip(outs, c.start_expect, oouts, START_NAMES):
            assert np.array_equal(a, want[sel]), f"{ctx}: intended Start {nm} at {np.flatnonzero(a != want[sel])[:8]}"
            assert np.array_equal(a, b), f"{ctx}: Start {nm} at {np.flatnonzero(a != b)[:8]}"
        assert_states_equal(e.store_state(), o.state(), G, P, L, ctx)


@pytest.mark.parametrize("mode", [TICK_LIGHT, TICK_FULL])
@pytest.mark.parametrize("P", lc.PEERS)
def test_negative_counts_gpu(P, mode):
    """counts[g] = -1 (include/mraft.h, mraft_start_and_tick): no error for an
    idle group (leader_peer -1), MRAFT_ITEM_BAD_SLOT with leader_peer in range
    (the tick still runs) and with leader_peer = P; nothing is appended."""
    c = lc.bad_slot_case(P)
    G, L, lp = c.G, c.L, c.leader_peer
    o = Oracle(G, P, L, c.state)
    with Engine(G, P, L) as e:
        e.load_state(c.state)
        e.set_tick_mode(mode)
        outs = _tick(e, o, lp, c.counts, G, P, L, f"bad slot P={P} mode={mode}")
    idx, term, isl, err = outs
    neg = c.counts < 0
    assert np.all(idx[neg] == -1) and np.all(term[neg] == -1) and np.all(isl[neg] == 0)
    assert np.all(err[neg & (lp < 0)] == 0)
    assert np.all(err[neg & (lp >= 0) & (lp < P)] == ITEM_BAD_SLOT)
    assert np.all(err[neg & (lp >= P)] == ITEM_BAD_SLOT)
    assert neg.sum() == 9 and len({int(x) for x in lp[neg]} & {-1, P}) == 2
    assert np.all(err[~neg] == 0) and np.all(isl[~neg] == 1)
    for a, b in zip(outs, c.start_expect):
        assert np.array_equal(a, b)
