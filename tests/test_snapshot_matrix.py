"""The directed cases of the item-level kernels (tests/snapshot_matrix_cases.py:
Snapshot, the InstallSnapshot gather, HandleInstallSnapshot, its reply fold,
persistence and Start) on the CPU, before any GPU sees them.

Per family: the plain Python model equals the C oracle on every output of the
family's script (outputs, item errors, flags, headers and terms, persist bits)
and on the whole state, `persist_dirty` and `log_head` included, after the
batch, after the follow-up and after every other call that can change it; and
every cell the family claims is present in the model's classification (`cells`
sees only the model's record: a cell taken out of a builder fails here by
name; no cell may be left out). MATRIX lists the cells one by one; the
families' claims together must be exactly that set. For the cross-path
families the oracle's tick equals the same tick composed from the oracle's
message-level calls, and the claimed situations are present in that
composition's record."""
import numpy as np
import pytest

import snapshot_matrix_cases as mc
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd._abi import G_ERROR, ITEM_NEED_SNAPSHOT

ITEM_FAMILIES = [n for n in mc.NAMES if mc.KIND[n] != "cross"]
CROSS = [n for n in mc.NAMES if mc.KIND[n] == "cross"]


def _matrix():
    m = set()
    m |= {"S.idx." + k for k in ("below", "eq_dummy", "dummy1", "mid", "eq_last", "beyond", "last_top")}
    m |= {"S.head.Lm1", "S.head.zero_exact", "S.head.past_wrap", "S.commit_below_dummy", "S.applied_below_dummy",
          "S.persist.moved3", "S.persist.unmoved0", "S.dup.first_wins_other_index", "S.slot.neg", "S.slot.gp",
          "S.batch_gt256", "S.pos255", "S.pos256"}
    m |= {"G.prev.dummy_m1", "G.prev.eq_dummy", "G.next0", "G.role.follower", "G.role.candidate", "G.peer.me",
          "G.peer.P", "G.peer.neg", "G.slot.neg", "G.slot.gp", "G.dterm.head0", "G.dterm.mid", "G.dterm.Lm1",
          "G.need_snapshot_iff_args"}
    m |= {f"H.term.{t}.{r}" for t in ("lt", "eq", "gt") for r in ("follower", "candidate", "leader")}
    m |= {"H.lii." + k for k in ("eq_commit", "commit1", "eq_last", "last1", "top", "past_domain")}
    m |= {"H.below_dummy", "H.below_dummy.newer_term", "H.slice0", "H.head.Lm1", "H.head.zero_exact",
          "H.head.past_wrap", "H.lit_differs", "H.voted.reset_gt", "H.voted.kept_eq", "H.hsnap", "H.persist.0",
          "H.persist.1", "H.persist.3", "H.srt.new_log_sets", "H.srt.slice_keeps0", "H.srt.slice_keeps1", "H.dup",
          "H.slot.neg", "H.slot.gp", "H.incoming_err"}
    m |= {"F.null_seg_begin", "F.explicit", "F.len0", "F.len1", "F.lenPm1", "F.len_gtPm1", "F.applied", "F.repeat_peer",
          "F.stepdown.first", "F.stepdown.middle", "F.stepdown.last", "F.stepdown.second_higher",
          "F.after_stepdown_ignored", "F.reply_eq_term", "F.reply_below_term", "F.args_below.leader",
          "F.args_above.leader", "F.nonleader_ignored.follower", "F.nonleader_ignored.candidate",
          "F.lowers_match_next", "F.bad.peer_me", "F.bad.peer_neg", "F.bad.peer_P", "F.bad.other_slot", "F.bad.lii.k0",
          "F.bad.lii.klast", "F.bad.stepdown_inside", "F.first_slot_oob", "F.dup_later", "F.lii.top", "F.nseg_gt64",
          "F.seg63", "F.seg64", "F.seg65"}
    m |= {f"P.read.n{c}.w{w}" for c in mc.ROW_LENS + ("L",) for w in mc.WRAPS}
    m |= {"P.read.iter2", "P.read.wrap_in_iter2", "P.read.unordered", "P.read.slot_twice", "P.read.cap_short"}
    m |= {f"P.restore.descent.{a}_{b}" for a, b in mc.DESCENTS}
    m |= {"P.restore.descent.last", "P.restore.descent.0_1_sorted", "P.restore.sorted", "P.restore.iter2",
          "P.restore.resets_all", "P.accept.L_terms"}
    m |= {"P.refuse." + c for c in ("slot_neg", "slot_gp", "last_lt_dummy", "dummy_neg", "off_neg", "off_past",
                                    "too_long", "dup")}
    m |= {"T.dup_other_count", "T.counts_null", "T.count0", "T.cross.first", "T.cross.middle", "T.cross.last",
          "T.top_above_clears", "T.top_eq_keeps"}
    m |= {"X.mixed", "X.is_stepdown", "X.is_stepdown_before_ae_success", "X.follower_panic", "X.slice_wraps",
          "X.masked_snapshot_dropped"}
    return m


MATRIX = _matrix()
_runs = {}


def _run(name):
    """(model, oracle) after the family's script; model == oracle checked on the way."""
    if name not in _runs:
        G, P, L, st, b, _ = mc.family(name)
        o, m = Oracle(G, P, L, st), mc.Model(G, P, L, st)
        assert np.array_equal(o.state()["terms_sorted"], st["terms_sorted"]), f"{name}: the builder's terms_sorted"
        got = mc.SCRIPTS[mc.KIND[name]](m, b, tick=False)
        want = mc.SCRIPTS[mc.KIND[name]](o, b, tick=False)
        mc.compare_outputs(got, want, f"{name}: model vs oracle", assert_states_equal, (G, P, L))
        assert_states_equal(m.state(), o.state(), G, P, L, f"{name}: model vs oracle")
        _runs[name] = (m, o)
    return _runs[name]


@pytest.mark.parametrize("name", ITEM_FAMILIES)
def test_model_equals_oracle_and_cells_present(name):
    m, _ = _run(name)
    claims = mc.family(name)[5]
    assert claims - mc.cells(m.trace) == set(), f"{name}: claimed cells the model does not find"


def test_claims_are_the_matrix():
    claimed = set()
    for name in mc.NAMES:
        claimed |= mc.family(name)[5]
    assert MATRIX - claimed == set(), "matrix cells no family claims"
    assert claimed - MATRIX == set(), "claims the matrix does not list"


def test_sizes_are_the_smallest():
    for name in mc.NAMES:
        G, P, L = mc.family(name)[:3]
        assert G <= 64 and P in (2, 3, 5, 8), name
        assert L in ((520, 515) if mc.KIND[name] in ("persist", "restore") else (16, 13)), name
    assert mc.family("grid300")[0] * mc.family("grid300")[1] == 300


@pytest.mark.parametrize("name", [n for n in ITEM_FAMILIES if mc.KIND[n] == "snapshot"])
def test_quirk_group_ticks_to_an_error(name):
    """commitIndex and lastApplied stay below the dummy Snapshot moved (the
    reference's quirk); the leader's next tick refuses the group."""
    G, P, L, st, b, _ = mc.family(name)
    o = Oracle(G, P, L, st)
    o.snapshot(b["slots"], b["index"])
    g = b["quirk_group"]
    s = g * P
    assert o.state()["commit_index"][s] < o.state()["dummy_index"][s] > o.state()["last_applied"][s]
    gf = o.replicate_tick(b["lp"])
    assert gf[g] == G_ERROR and not np.delete(gf, g).any()


@pytest.mark.parametrize("name", [n for n in ITEM_FAMILIES if mc.KIND[n] == "gather"])
def test_need_snapshot_exactly_where_args(name):
    """mraft_gather_append_args answers NEED_SNAPSHOT exactly on the items the
    InstallSnapshot gather produced args for: model and oracle alike."""
    G, P, L, st, b, _ = mc.family(name)
    for eng in (Oracle(G, P, L, st), mc.Model(G, P, L, st)):
        ia, ierr = eng.gather_install_snapshot_args(b["slots"], b["peers"])
        _, aerr = eng.gather_append_args(b["slots"], b["peers"])
        made = (ierr == 0) & (ia["slot"] >= 0)
        assert np.array_equal(made, aerr == ITEM_NEED_SNAPSHOT) and made.any() and (~made & (ierr == 0)).any()


@pytest.mark.parametrize("name", [n for n in ITEM_FAMILIES if mc.KIND[n] in ("restore", "handle", "fold")])
def test_refused_items_leave_their_replica_untouched(name):
    G, P, L, st, b, _ = mc.family(name)
    o = Oracle(G, P, L, st)
    kind = mc.KIND[name]
    if kind == "restore":
        err = o.restore(b["hdr"], b["terms"])
        slots, ok = b["hdr"]["slot"], set(b["hdr"]["slot"][err == 0].tolist())
    elif kind == "handle":
        _, _, err = o.handle_install_snapshot(b["args"])
        slots, ok = b["args"]["slot"], set(b["args"]["slot"][err == 0].tolist())
    else:
        _, err = o.process_install_snapshot_replies(b["items"], b["seg"])
        sb = np.arange(len(b["items"]) + 1) if b["seg"] is None else b["seg"]
        first = sb[:-1][sb[:-1] < sb[1:]]
        slots, err = b["items"]["slot"][first], err[first]
        ok = set(slots[err == 0].tolist())
    after, n = o.state(), 0
    for s in set(slots[err != 0].tolist()) - ok:
        if 0 <= s < G * P:
            n += 1
            for k, v in st.items():
                w = L if k == "log_term" else P if k in ("match_index", "next_index") else 1
                assert np.array_equal(after[k][s * w:(s + 1) * w], v[s * w:(s + 1) * w]), (name, k, s)
    assert n >= 3, name


def test_persistence_rows_reach_the_second_iterations():
    """Rows of more than 256 terms (mraft_device.h kChunk) are read out and
    restored, with the ring's wrap inside the second iteration; the descents of
    the restore rows stand at the 64-pair edges wave_terms_sorted ballots by."""
    for name in ("persist520", "persist515"):
        m, _ = _run(name)
        rows = [R for R in m.trace if R["op"] == "read_row"]
        assert max(R["cnt"] for R in rows) == mc.family(name)[2] > 2 * mc.KCHUNK
        assert any(R["cnt"] > mc.KCHUNK and R["w"] == mc.KCHUNK + 1 for R in rows)
        assert sum(R["cnt"] > mc.KCHUNK for R in [R for R in m.trace if R["op"] == "restore"]) >= 20
    for name in ("restore520", "restore515"):
        m, _ = _run(name)
        got = {tuple(R["descents"]) for R in m.trace
               if R["op"] == "restore" and R["cls"] == "restored" and R["srt"] == 0}
        assert {(a,) for a, _ in mc.DESCENTS} <= got


@pytest.mark.parametrize("name", ["persist520", "persist515"])
def test_tick_after_restore_replicates_to_restored_followers(name):
    """restore(read_persistent(x)), then one full tick: every group's leader
    (left out of the restore) sends to followers whose logs are the restored
    rows, and every one of them answers with a conflict found in such a row."""
    from multiraft_amd._abi import G_ACTIVE
    G, P, L, st, b, _ = mc.family(name)
    o = Oracle(G, P, L, st)
    rc, hdr, terms = mc.read_persistent_raw(o, b["slots"], b["need"])
    assert rc == 0 and not o.restore(hdr, terms)[hdr["slot"] != hdr["slot"][5]].any()
    before = o.store_state()
    gf = o.replicate_tick(b["lp"])
    assert (gf & G_ACTIVE).all()
    after = o.state()
    lead = np.arange(G) * P + P - 1
    nx0, nx1 = before["next_index"].reshape(G * P, P)[lead], after["next_index"].reshape(G * P, P)[lead]
    assert (nx0 != nx1).any(axis=1).all()
    assert (after["current_term"][b["slots"]] == 70).all()


@pytest.mark.parametrize("name", CROSS)
def test_cross_path_groups(name):
    """The oracle's tick equals its message-level calls in the tick's order,
    and the claimed situations are in that composition's record."""
    G, P, L, st, b, claims = mc.family(name)
    exp = mc.cross_expected(Oracle, name)
    assert np.array_equal(exp["plain"][0], exp["composed"][0]), (exp["plain"][0], exp["composed"][0])
    assert_states_equal(exp["plain"][1], exp["composed"][1], G, P, L, f"{name}: tick vs message path")
    assert claims - mc.cross_cells(name, exp) == set(), f"{name}: claimed situations not present"
    masked = list(b["names"]).index("masked")
    assert not np.array_equal(exp["masked"][1]["dummy_index"], exp["plain"][1]["dummy_index"])
    assert np.array_equal(np.delete(exp["masked"][0], masked), np.delete(exp["plain"][0], masked))
