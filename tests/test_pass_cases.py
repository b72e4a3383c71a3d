"""The directed fixtures of the streaming merge pass (tests/pass_cases.py)
against the CPU oracle alone, before any GPU sees them.

Per family and form: the oracle's tick (raft_append_entry.go:20-162) and its
message path (gather -> HandleAppendEntries by reference and by value -> fold)
run on the built state. Every group is active; only the groups built to be
rejected carry MRAFT_G_LOG_FULL / MRAFT_ITEM_LOG_FULL; every follower's reply
class, first written Index and resulting last Index are the builder's intended
ones; terms_sorted stays sound. Then `pass_cases.geometry`, which sees the
state arrays only, must find every cell the family claims (set inclusion: a
cell taken out of the builder fails here), and the group counts are pinned."""
import numpy as np
import pytest

import pass_cases as pc
from message_cases import all_follower_items, external_entries, results_of
from oracle_lib import Oracle, assert_states_equal, assert_terms_sorted_sound, logical_logs

from multiraft_amd._abi import AE_ENTRIES_SORTED, G_ACTIVE, G_LOG_FULL, ITEM_LOG_FULL, ITEM_NEED_SNAPSHOT

M_FORMS = ("vec", "mis1", "odd")
W_FORMS = pc.FORMS
S_FORMS = ("vec", "mis2", "odd")
# groups per case
COUNTS = {"M-vec": 1074, "M-mis1": 1659, "M-odd": 1659, "W-vec": 384, "W-mis1": 408, "W-mis2": 408, "W-mis3": 408, "W-odd": 1020, "W-bound": 1020,
          "F-vec": 374, "F-mis1": 383, "F-mis2": 383, "F-mis3": 383, "F-odd": 383, "F-bound": 383,
          "N-P3": 90, "N-P5": 180, "N-P8": 90, "S-vec": 323, "S-mis2": 356, "S-odd": 356, "C-P2": 78, "C-P5": 39,
          "D-vec": 96, "D-mis1": 96, "D-odd": 96, "V-vec": 472}


def _written(c, pre, post):
    """Per group {peer: (first Index written or None, last)} from two state
    images: an Index of [prev + 1, new last] counts as written where it lies
    past the old last or its term changed."""
    G, P, L = c.G, c.P, c.L
    a, b = logical_logs(pre, G, P, L), logical_logs(post, G, P, L)
    out = []
    for g in range(G):
        ld = g * P + c.leader_peer[g]
        d = {}
        for j in c.expect[g]:
            f = g * P + j
            if pre["dummy_index"][f] != post["dummy_index"][f]:
                d[j] = (None, None)     # a snapshot was installed
                continue
            dm, ol, nl = int(pre["dummy_index"][f]), int(pre["last_index"][f]), int(post["last_index"][f])
            prev = int(pre["next_index"][ld * P + j]) - 1
            first = None
            for i in range(max(prev + 1, dm), nl + 1):
                if i > ol or a[f, i - dm] != b[f, i - dm]:
                    first = i
                    break
            d[j] = (first, nl)
        out.append(d)
    return out


def _check_outcomes(c, got, ctx, tick):
    for g in range(c.G):
        for j, (cls, first, last, _) in c.expect[g].items():
            if cls == "snap":
                if not tick:   # the AppendEntries path leaves it alone
                    assert got[g][j][1] is not None, (ctx, g, j)
                continue
            assert got[g][j] == (first, last), f"{ctx}: group {g} ({c.kinds[g]}) peer {j}: {got[g][j]} != {(first, last)}"


def _oracle_tick(c):
    ctx = f"{c.name} tick"
    o = Oracle(c.G, c.P, c.L, c.state)
    assert np.array_equal(o.state()["terms_sorted"], c.state["terms_sorted"]), ctx
    gf = o.replicate_tick(c.leader_peer)
    assert np.all(gf & G_ACTIVE), f"{ctx}: inactive groups {np.flatnonzero((gf & G_ACTIVE) == 0)[:8]}"
    assert np.array_equal((gf & G_LOG_FULL) != 0, c.rejected), f"{ctx}: MRAFT_G_LOG_FULL"
    assert_terms_sorted_sound(o.state(), c.G, c.P, c.L, ctx)
    _check_outcomes(c, _written(c, c.state, o.state()), ctx, True)


def _oracle_messages(c, by):
    G, P, L = c.G, c.P, c.L
    ctx = f"{c.name} messages by {by}"
    o = Oracle(G, P, L, c.state)
    slots, peers = all_follower_items(c.leader_peer, G, P)
    args, gerr = o.gather_append_args(slots, peers)
    ok = gerr == 0
    if by == "value":
        ext, buf = external_entries(args, ok, o.state(), L, misalign=True)
        batch = ext[ok]
    else:
        batch, buf = args[ok], None
    rep, herr = o.handle_append_entries(batch, buf)
    it = iter(range(int(ok.sum())))
    for k in range(len(slots)):
        g, j = int(slots[k]) // P, int(peers[k])
        cls, _, _, ci = c.expect[g][j]
        if cls == "snap":
            assert gerr[k] == ITEM_NEED_SNAPSHOT, (ctx, g, j)
            continue
        assert gerr[k] == 0, (ctx, g, j)
        r = next(it)
        what = f"{ctx}: group {g} ({c.kinds[g]}) peer {j} {cls}: reply {rep[r]}, err {herr[r]}"
        if cls == "full":
            assert herr[r] == ITEM_LOG_FULL, what
            continue
        assert herr[r] == 0, what
        assert rep["success"][r] == (cls in ("merge", "hb")), what
        if cls == "stale":
            assert rep["term"][r] > args["term"][k], what
        elif ci is not None:
            assert rep["conflict_index"][r] == ci, what
    res, seg = results_of(slots[ok], peers[ok], args[ok], rep, herr, G, P)
    o.process_append_replies(res, seg)
    assert_terms_sorted_sound(o.state(), G, P, L, ctx)
    _check_outcomes(c, _written(c, c.state, o.state()), ctx, False)
    return o.state()


def _check_case(c):
    assert 0 < c.G <= 2048, c.name
    assert c.G == COUNTS[c.name], (c.name, c.G)
    assert_terms_sorted_sound(c.state, c.G, c.P, c.L, c.name)
    _oracle_tick(c)
    a = _oracle_messages(c, "reference")
    b = _oracle_messages(c, "value")
    assert_states_equal(a, b, c.G, c.P, c.L, f"{c.name}: by reference vs by value")


def _geo(c):
    return pc.geometry(c.state, c.leader_peer, c.P, c.L, log_off=1 if c.form == "bound" else 0)


def _dead_word(c, f, i):
    st = c.state
    return int(st["log_term"].reshape(-1, c.L)[f, (int(st["log_head"][f]) + i - int(st["dummy_index"][f])) % c.L])


def _m_cells(c):
    """Per (kind, fit): the sets of line offsets, rels and nend tags seen,
    and for family W the (leader wrap, follower wrap) pairs; kind and fit are
    re-derived from the state, not read from the builder's strings alone."""
    seen = {}
    for g, geo in enumerate(_geo(c)):
        assert geo["vec"] == (c.form == "vec"), (c.name, g)
        (j, d), = [(j, d) for j, d in geo["fols"].items() if d["cls"] == "merge"]
        f = g * c.P + j
        L, nend = c.L, geo["nend"]
        if d["m"] is None:
            kind, m = "match_longer", d["cend"] - 1
            assert d["cend"] == nend and d["flast"] >= nend - 1
        elif d["m"] < d["cend"]:
            kind, m = "mismatch", d["m"]
        else:
            m = d["m"]
            assert m == d["cend"] == d["flast"] + 1 < nend
            # the dead slot at m: the leader's term there (tail) or poison (beyond)
            w = _dead_word(c, f, m) if m - d["fdummy"] <= L - 1 else None
            kind = "tail" if w == _dead_word(c, g * c.P + c.leader_peer[g], m) else "beyond"
            assert kind == "tail" or w in (pc.POISON, None)
            if w is None:   # the follower's ring is full: no dead slot tells the two apart
                kind = c.kinds[g].split("/")[0]
                assert kind in ("tail", "beyond")
        room = (nend - 1) - d["fdummy"]
        fit = "over" if room == L else "exact" if room == L - 1 else "normal"
        assert d["full"] == (fit == "over") and room <= L
        assert c.kinds[g] == f"{kind}/{fit}", (c.name, g, c.kinds[g], kind, fit)
        # the decision point the grid rules find is the one the builder intends (and the oracle confirms)
        assert c.expect[g][j][1] == (m if kind != "match_longer" and fit != "over" else None), (c.name, g)
        s = seen.setdefault((kind, fit), dict(off=set(), rel=set(), nend=set(), wrap=set()))
        s["off"].add(geo["line"])
        rel = geo["pos"](m)[0]
        s["rel"].add(rel)
        if m == d["start"]:
            s["rel"].add("first")
        s["nend"] |= pc.nend_tags(geo, m)
        o = geo["origin"]
        s["wrap"].add((None if d["lwrap"] is None else d["lwrap"] - o, None if d["fwrap"] is None else d["fwrap"] - o))
    return seen


def _assert_m_cells(c, offs, rels, fits_rels):
    seen = _m_cells(c)
    for kind in pc.KINDS:
        s = seen[(kind, "normal")]
        if c.L % pc.LINE == 0:   # (L = 1023: the rows start anywhere in a line, and the dword origin ignores it)
            assert set(offs) <= s["off"], (c.name, kind, "line offsets")
        assert set(rels) <= s["rel"], (c.name, kind, "rels", set(rels) - s["rel"])
        # match_longer: the compared range ends with the entries, nend is m + 1 by definition
        want = {"m+1"} if kind == "match_longer" else set(pc.NENDS)
        assert want <= s["nend"], (c.name, kind, "nend", want - s["nend"])
        if kind != "match_longer":   # the kinds that write: exact fit and one over
            for fit in ("exact", "over"):
                s = seen[(kind, fit)]
                assert c.L % pc.LINE or set(offs) <= s["off"], (c.name, kind, fit)
                assert set(fits_rels) <= s["rel"], (c.name, kind, fit)
        else:
            assert (kind, "exact") not in seen and (kind, "over") not in seen
    return seen


@pytest.mark.parametrize("form", M_FORMS)
def test_family_m(form):
    c = pc.case("M", form)
    _check_case(c)
    _assert_m_cells(c, pc.OFFS, pc.m_rels(form), pc.m_rels(form))


@pytest.mark.parametrize("form", pc.FORMS)
def test_family_f(form):
    c = pc.case("F", form)
    assert c.L == (1023 if form == "odd" else 1024)
    _check_case(c)
    _assert_m_cells(c, pc.F_OFFS, pc.F_RELS, pc.F_RELS)
    if form.startswith("mis"):
        st, P = c.state, c.P
        ld = np.arange(c.G) * P + c.leader_peer
        fo = np.arange(c.G) * P + (1 - c.leader_peer)
        diff = ((st["log_head"][fo] - st["dummy_index"][fo]) - (st["log_head"][ld] - st["dummy_index"][ld])) % 4
        assert np.all(diff == int(form[3])), form
    if form == "bound":   # the same state on a 16-B aligned log would take the dwordx4 form
        assert all(g["vec"] for g in pc.geometry(c.state, c.leader_peer, c.P, c.L))


@pytest.mark.parametrize("form", W_FORMS)
def test_family_w(form):
    c = pc.case("W", form)
    _check_case(c)
    seen = _m_cells(c)
    for kind in pc.KINDS:
        s = seen[(kind, "normal")]
        assert set(pc.w_wraps(form)) <= s["wrap"], (form, kind, set(pc.w_wraps(form)) - s["wrap"])
        # (dword forms: the origin is plo itself, its line offset places nothing)
        assert form != "vec" or set(pc.W_OFFS) <= s["off"], (form, kind)
        if kind == "match_longer":   # its entries end at m
            assert set(pc.W_RELS_LONGER) <= s["rel"], (form, kind)
        else:
            assert set(pc.W_RELS) <= s["rel"], (form, kind)
            assert s["nend"] <= {"E+256", "E+257", "E+259"} and len(s["nend"]) == 3
    if form in ("odd", "bound"):     # every residue mod 4, on either side
        for side in (0, 1):
            assert {w[side] % 4 for w in pc.w_wraps(form) if w[side] is not None} == {0, 1, 2, 3}


@pytest.mark.parametrize("P", pc.N_PEERS)
def test_family_n(P):
    c = pc.case("N", "vec", P)
    _check_case(c)
    tags, lps, beside = set(), set(), set()
    for g, geo in enumerate(_geo(c)):
        pos = geo["pos"]
        mg = {j: d for j, d in geo["fols"].items() if d["cls"] == "merge"}
        assert mg, g
        lps.add(int(c.leader_peer[g]))
        beside |= {d["cls"] for d in geo["fols"].values()}
        if {0, 1, 2} <= {pos(d["start"])[1] for d in mg.values()}:
            tags.add("starts in chunks 0, 1, 2")
        for a in mg.values():
            for b in mg.values():
                if a is b:
                    continue
                if a["m"] is not None and pos(a["m"])[1] < pos(b["start"])[1]:
                    tags.add("one done before another starts")
                if a["m"] is not None and a["m"] < a["cend"] and pos(a["m"])[0] % pc.CHUNK == pc.CHUNK - 1 \
                        and pos(b["cend"] - 1)[1] == pos(a["m"])[1] and b["start"] < b["cend"]:
                    tags.add("mismatch on the last entry of the chunk where another's range ends")
                if a["full"] and not b["full"]:
                    tags.add("one full, others fit")
        if not geo["vec"]:
            mis = [((d["fhead"] - d["fdummy"]) - (c.state["log_head"][g * P + c.leader_peer[g]]
                                                   - c.state["dummy_index"][g * P + c.leader_peer[g]])) % 4 != 0
                   for d in mg.values()]
            if sum(mis) == 1 and len(mis) > 1:
                tags.add("dword by one follower")
    assert lps == {0, P // 2, P - 1}
    assert {"merge", "hb", "stale", "below", "beyond", "snap"} <= beside
    want = {"starts in chunks 0, 1, 2", "one done before another starts", "one full, others fit",
            "mismatch on the last entry of the chunk where another's range ends"}
    if P == 3:   # two followers: three start chunks need three
        want.discard("starts in chunks 0, 1, 2")
    if P == 5:
        want.add("dword by one follower")
    assert want <= tags, (P, want - tags)


@pytest.mark.parametrize("form", S_FORMS)
def test_family_s(form):
    c = pc.case("S", form)
    _check_case(c)
    tags, rels, late = set(), set(), set()
    for g, geo in enumerate(_geo(c)):
        merging = any(d["cls"] == "merge" for d in geo["fols"].values())
        # (with no merging follower nothing constrains the form: dwordx4 wherever L % 4 == 0)
        assert geo["vec"] == (form == "vec" or (not merging and c.L % 4 == 0)), g
        ld = g * c.P + c.leader_peer[g]
        sc = geo["scan"]
        if sc is None:
            assert geo["settled"] and c.state["terms_sorted"][ld] == 1 and c.kinds[g] == "settled", g
            tags.add("settled")
            continue
        assert c.state["terms_sorted"][ld] == 0, g
        slo, shi, hit = sc["slo"], sc["shi"], sc["hit"]
        if sc["late"]:   # a maybe_full group: wave_scan_down_eq after the pass
            late |= {(shi - slo + 1, t) for t, at in (("none", None), ("slo", slo), ("shi", shi)) if hit == at}
            if hit is not None and slo < hit < shi:
                late.add((shi - slo + 1, "mid"))
            continue
        mg = [d for d in geo["fols"].values() if d["cls"] == "merge"]
        if hit is None:
            tags.add("no hit")
        else:
            rels.add(geo["pos"](hit)[0])
            if hit == geo["plo"]:
                rels.add("first")
            tags |= {"at slo"} if hit == slo else set()
            tags |= {"at shi"} if hit == shi else set()
            if mg and hit >= max(d["cend"] for d in mg) + pc.CHUNK:
                tags.add("copy-only region")
        if mg and slo < min(d["start"] for d in mg):
            tags.add("window below every start")
            assert geo["plo"] == slo
        if not mg:
            tags.add("no merging follower")
            assert geo["phi"] == shi
    assert set(pc.RELS) <= rels, (form, set(pc.RELS) - rels)
    assert {"settled", "no hit", "at slo", "at shi", "copy-only region", "window below every start",
            "no merging follower"} <= tags, tags
    for n in pc.S_FULL_LENS:
        assert {(n, "none"), (n, "slo"), (n, "shi")} <= late, (n, late)
        assert n <= 2 or (n, "mid") in late, n


@pytest.mark.parametrize("P", [2, 5])
def test_family_c(P):
    c = pc.case("C", "vec", P)
    _check_case(c)
    cells, widths = set(), set()
    for g, geo in enumerate(_geo(c)):
        assert geo["cscan"], g
        cells |= set(geo["cscan"].values())
        widths.add(len(geo["cscan"]))
    if P == 2:
        assert {(r, b, w) for r in pc.C_RUNS for b in pc.C_BREAKERS for w in (False, True)} <= cells
    else:
        assert widths == {2, 3, 4}
        assert {r for r, _, _ in cells} == set(pc.C_RUNS) and {b for _, b, _ in cells} == set(pc.C_BREAKERS)
        assert {w for _, _, w in cells} == {False, True}


@pytest.mark.parametrize("form", pc.D_FORMS)
def test_family_d(form):
    """One descent in the shipped entries, at every position of the list, with
    the follower's compare ending nowhere / in chunk 0 / in chunk 1 and its
    dummy at prev or below; and the oracle's verdict on the flag, as gathered
    (truthful: the leader's own proof) and forced on (a false claim wherever
    the descent lies inside the message)."""
    c = pc.case("D", form)
    _check_case(c)
    G, P, L = c.G, c.P, c.L
    cells, inside = set(), np.zeros(G, bool)
    for g, geo in enumerate(_geo(c)):
        assert geo["vec"] == (form == "vec") and len(geo["desc"]) <= 1, g
        (d,) = [d for d in geo["fols"].values() if d["cls"] == "merge"]
        keep = "none" if d["cend"] == d["start"] else f"chunk{geo['pos'](d['cend'] - 1)[1]}"
        atprev = d["fdummy"] == d["start"] - 1
        if not geo["desc"]:
            tags = {"absent"}
        else:
            x = geo["desc"][0]
            rel = geo["pos"](x)[0]
            inside[g] = x >= d["start"]
            tags = {t for t, hit in (("first", x == d["start"]), ("second", x == d["start"] + 1), ("lane64", rel == pc.WAVE),
                                     ("lane128", rel == 2 * pc.WAVE), ("chunk", rel == pc.CHUNK),
                                     ("last", x == geo["nend"] - 1), ("outside", x < d["start"])) if hit}
            assert tags, (g, x)
        cells |= {(t, keep, atprev) for t in tags}
    assert {(t, k, a) for t in pc.D_POS for k in ("none", "chunk0", "chunk1") for a in (False, True)} <= cells
    fo = np.arange(G) * P + (1 - c.leader_peer)
    slots, peers = all_follower_items(c.leader_peer, G, P)
    for forced in (False, True):
        for by in ("reference", "value"):
            o = Oracle(G, P, L, c.state)
            args, gerr = o.gather_append_args(slots, peers)
            assert not gerr.any()
            # as gathered the flag is the leader's proof: set only where its log has no descent at all
            assert np.array_equal((args["flags"] & AE_ENTRIES_SORTED) != 0,
                                  np.array([not geo["desc"] for geo in _geo(c)]))
            if forced:
                args["flags"] |= AE_ENTRIES_SORTED
            buf = None
            if by == "value":
                args, buf = external_entries(args, gerr == 0, o.state(), L, misalign=True)
            rep, herr = o.handle_append_entries(args, buf)
            assert not herr.any() and rep["success"].all()
            assert_terms_sorted_sound(o.state(), G, P, L, f"{c.name} forced {forced} by {by}")
            # forced on: honoured unless the descent lies inside the message (prevLogTerm > entry 0 included)
            want = ~inside if forced else np.array([not geo["desc"] for geo in _geo(c)])
            assert np.array_equal(o.state()["terms_sorted"][fo] != 0, want), (form, forced, by)


def _value_run(c, layout):
    """The oracle's handler on the layout's buffer: the same replies and the
    same state as by reference. Returns (args, ok, per-item geometry)."""
    G, P, L = c.G, c.P, c.L
    slots, peers = all_follower_items(c.leader_peer, G, P)
    o, o2 = Oracle(G, P, L, c.state), Oracle(G, P, L, c.state)
    args, gerr = o.gather_append_args(slots, peers)
    ok = gerr == 0
    merging = pc.merging_items(c, slots, peers)
    a2, buf, base_off = pc.value_layout(args, ok, o.state(), L, layout, eligible=merging)
    assert base_off == (int(layout[-1]) if layout.startswith("word0") else 0)
    geo = pc.value_geometry(a2, ok, c.state, L, len(buf), base_off)
    rep, herr = o.handle_append_entries(a2[ok], buf)
    rep2, herr2 = o2.handle_append_entries(args[ok], None)
    assert np.array_equal(rep, rep2) and np.array_equal(herr, herr2), (c.name, layout)
    assert_states_equal(o.state(), o2.state(), G, P, L, f"{c.name} {layout}")
    return a2, ok, geo, merging, slots


def test_value_layouts():
    """Family V: the buffer layouts over the V (one message per leader) and N
    (P = 5) states really hold the cells they are named for."""
    c = pc.case("V", "vec")
    _check_case(c)
    _, _, geo, mg, _ = _value_run(c, "residue")
    seen = {(d["residue"], d["aligned"]) for d, m in zip(geo, mg) if m and d}
    assert seen == {(r, a) for r in range(4) for a in (False, True)}
    assert all(d["head_ok"] and d["tail_ok"] for d in geo if d)
    _, _, geo, mg, _ = _value_run(c, "lastword")
    cut = [j for j, d in enumerate(geo) if d and not d["tail_ok"]]
    assert len(cut) == 1 and mg[cut[0]] and geo[cut[0]]["aligned"] and geo[cut[0]]["head_ok"]
    assert all(d["vec"] for j, d in enumerate(geo) if d and j != cut[0])
    for r in (1, 2, 3):
        a2, _, geo, mg, _ = _value_run(c, f"word0-{r}")
        cut = [j for j, d in enumerate(geo) if d and not d["head_ok"]]
        assert len(cut) == 1 and mg[cut[0]] and geo[cut[0]]["aligned"] and geo[cut[0]]["tail_ok"]
        assert a2["entries_offset"][cut[0]] == 0
        assert all(d["vec"] for j, d in enumerate(geo) if d and j != cut[0])
    c = pc.case("N", "vec", 5)
    a2, ok, geo, mg, slots = _value_run(c, "shared")
    sizes = set()
    for s in np.unique(slots):
        it = [j for j in np.flatnonzero(slots == s) if geo[j] and mg[j]]
        ends = {int(a2["entries_offset"][j] + a2["n_entries"][j]) for j in it}
        assert len(ends) <= 1, s           # one source range, one end
        sizes.add(len(it))
    assert {2, 3, 4} <= sizes
    assert {d["residue"] for d in geo if d} == {0, 1, 2, 3}
