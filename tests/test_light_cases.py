"""The directed light-tick fixtures (tests/light_cases.py) against the CPU
oracle alone, before any GPU sees them: the oracle's Start (raft.go:90-104)
over the leader slots where the case sets counts, then its tick
(raft_append_entry.go:20-162).

Every group is active; a group tagged as settling in the light launch ends
with every follower at the leader's last Index and the leader's nextIndex /
matchIndex words at last + 1 / last (the followers a case builds ahead of the
leader or with a longer log excepted, by the case's own per-peer mask);
Start's outputs and errors are the ones the generator intends; the tags equal
an independent restatement of the settle rule over the state arrays; and
every family's counts of light and listed groups are the pinned numbers."""
import numpy as np
import pytest

import light_cases as lc
from oracle_lib import Oracle, assert_terms_sorted_sound

from multiraft_amd._abi import G_ACTIVE, ITEM_BAD_SLOT, ITEM_LOG_FULL

# (light, listed) groups of the mixed case per capacity 37, 64, 99, 256. E grows with P (its few-successes
# groups need P >= 4, one set per success count 1 .. P/2 - 1); every other family is the same for every P.
COUNTS = {
    "A": ((49, 0), (112, 0), (176, 5), (176, 5)),
    "B": ((167, 18), (188, 18), (192, 18), (192, 18)),
    "C": ((32, 16), (32, 16), (36, 16), (36, 16)),
    "D": ((93, 8),) * 4,
    "F": ((36, 36),) * 4,
}
E_PROBE = (21, 3)                       # P < 4: the probe groups only
E_FEW = (2, 3, 4, 4)                    # spans 5, 9, 33, 64 that fit capacity 37, 64, 99, 256
C_TOP = 18


def _expected_counts(family, P, L):
    k = lc.CAPACITIES.index(L)
    if family != "E":
        return COUNTS[family][k]
    # per span and success count: three wrap offsets each of two light and two listed shapes
    few = E_FEW[k] * max(0, P // 2 - 1) * 3 * 2 if P >= 4 else 0
    return E_PROBE[0] + few, E_PROBE[1] + few


def _check_case(c):
    G, P, L = c.G, c.P, c.L
    ctx = f"{c.name} P={P} L={L}"
    assert 0 < G <= 1024, ctx
    assert_terms_sorted_sound(c.state, G, P, L, ctx)
    assert np.array_equal(lc.settle_rule(c.state, P, L, c.leader_peer, c.counts), c.expect_listed), \
        f"{ctx}: tags differ from the restated rule"
    o = Oracle(G, P, L, c.state)
    assert np.array_equal(o.state()["terms_sorted"], c.state["terms_sorted"]), f"{ctx}: terms_sorted as loaded"
    if c.counts is None:
        assert c.start_expect is None
        gf = o.replicate_tick(c.leader_peer)
    else:
        gf, outs = lc.oracle_start_and_tick(o, c.leader_peer, c.counts, G, P)
        for a, b, name in zip(outs, c.start_expect, ("index", "term", "is_leader", "err")):
            assert np.array_equal(a, b), f"{ctx}: Start {name}: {np.flatnonzero(a != b)[:8]}"
    assert np.all(gf & G_ACTIVE), f"{ctx}: inactive groups {np.flatnonzero(~(gf & G_ACTIVE).astype(bool))[:8]}"
    st = o.state()
    last = st["last_index"].reshape(G, P)
    ld = np.arange(G) * P + c.leader_peer
    llast = st["last_index"][ld]
    nx = st["next_index"].reshape(G * P, P)[ld]
    mt = st["match_index"].reshape(G * P, P)[ld]
    light = ~c.expect_listed[:, None]
    app = light & (c.peer_kind == lc.PEER_APPEND)
    upd = light & ((c.peer_kind == lc.PEER_APPEND) | (c.peer_kind == lc.PEER_EXTRA))
    assert np.array_equal(last[app], np.broadcast_to(llast[:, None], (G, P))[app]), f"{ctx}: followers' last"
    assert np.array_equal(nx[upd], np.broadcast_to(llast[:, None] + 1, (G, P))[upd]), f"{ctx}: nextIndex"
    assert np.array_equal(mt[upd], np.broadcast_to(llast[:, None], (G, P))[upd]), f"{ctx}: matchIndex"
    return gf


@pytest.mark.parametrize("L", lc.CAPACITIES)
@pytest.mark.parametrize("family", lc.FAMILIES)
def test_family_against_oracle(family, L):
    for P in lc.PEERS:
        got = lc.cases(family, P, L)
        names = [c.name for c in got]
        assert names == [f"{family}-mixed", f"{family}-light"] + (["C-top-light"] if family == "C" else [])
        mixed, light = got[0], got[1]
        for c in got:
            assert (c.P, c.L, c.family) == (P, L, family)
            _check_case(c)
        exp = _expected_counts(family, P, L)
        assert (mixed.n_light, mixed.n_listed) == exp, (family, P, L)
        assert (light.n_light, light.n_listed) == (exp[0], 0), (family, P, L)
        # the light case is the mixed one without its listed groups
        assert [k for k, x in zip(mixed.kinds, mixed.expect_listed) if not x] == light.kinds
        if family == "C":
            assert (got[2].n_light, got[2].n_listed) == (C_TOP, 0)


def test_spans_and_wraps_family_a():
    """Family A holds every span of the issue's list with the ring's wrap at
    every offset 0 .. n-1 of the copied run, on the leader's side and, across
    the groups, on the slowest follower's side."""
    P, L = 5, 99
    c = lc.case("A-light", P, L)
    st = c.state
    seen = {}
    for g in range(c.G):
        ld = g * P + c.leader_peer[g]
        for j in range(P):
            if j == c.leader_peer[g]:
                continue
            f = g * P + j
            prev = st["next_index"][ld * P + j] - 1
            n = st["last_index"][ld] - prev
            rd = (L - (st["log_head"][ld] + prev + 1 - st["dummy_index"][ld])) % L   # entries before the read wraps
            wr = (L - (st["log_head"][f] + prev + 1 - st["dummy_index"][f])) % L
            s = seen.setdefault(int(n), (set(), set()))
            s[0].add(int(rd) if rd < n else -1)
            s[1].add(int(wr) if wr < n else -1)
    for n in lc.A_SPANS:
        assert set(range(n)) <= seen[n][0], (n, "read side")
        assert set(range(n)) <= seen[n][1], (n, "write side")


def test_start_outcomes_family_c():
    """Family C's Start outcomes: both sides of the ring's capacity and of
    the Index domain are present, with the errors the generator intends."""
    for L in lc.CAPACITIES:
        mixed, _, top = lc.cases("C", 5, L)
        err = mixed.start_expect[3]
        fits = np.array([k == "ringfits" for k in mixed.kinds])
        full = np.array([k == "ringfull" for k in mixed.kinds])
        assert fits.sum() == full.sum() > 0
        assert np.all(err[full] == ITEM_LOG_FULL) and np.all(err[fits] == 0) and np.all(mixed.start_expect[2][fits] == 1)
        terr = top.start_expect[3]
        kinds = np.array(top.kinds)
        assert np.all(terr[kinds == "topfits"] == 0) and np.all(terr[kinds != "topfits"] == ITEM_LOG_FULL)
        ld = np.arange(top.G) * 5 + top.leader_peer
        end = top.state["last_index"][ld].astype(np.int64) + top.counts
        assert np.all(end[kinds == "topfits"] == lc.INDEX_TOP) and np.all(end[kinds == "topfull"] == lc.INDEX_TOP + 1)
        assert np.all(end[kinds == "topringfull"] == lc.INDEX_TOP)


def test_tiny_and_bad_slot_cases():
    for G in (1, 7, 9, 31, 33, 255):
        for P in (2, 5, 8):
            light, listed = lc.tiny_cases(G, P)
            assert light.G == listed.G == G
            assert light.n_listed == 0 and listed.n_listed == G
            _check_case(light)
            _check_case(listed)
    for P in lc.PEERS:
        c = lc.bad_slot_case(P)
        g = np.arange(c.G)
        assert np.all(c.counts[g % 4 < 3] == -1)
        assert np.all(c.start_expect[3][g % 4 == 0] == 0) and np.all(c.leader_peer[g % 4 == 0] == -1)
        assert np.all(c.start_expect[3][(g % 4 == 1) | (g % 4 == 2)] == ITEM_BAD_SLOT)
        o = Oracle(c.G, P, c.L, c.state)
        _, outs = lc.oracle_start_and_tick(o, c.leader_peer, c.counts, c.G, P)
        for a, b in zip(outs, c.start_expect):
            assert np.array_equal(a, b)
