"""The directed cases of the reply fold (tests/fold_cases.py) on the CPU,
before any GPU sees them.

Per family: the plain Python model of the fold equals the C oracle (flags,
item errors, commit, term, role, match / next: the whole state), on the
family's batch and on the follow-up batch the GPU file folds second; the
oracle agrees with the builder's terms_sorted; and every cell the family
claims is present in the model's classification of that batch (`cells`, which
sees only the model's record: a cell taken out of a builder fails here by
name). MATRIX below lists the cells of A-E one by one; the families' claims
together must be exactly that set. The call-level claims of the default build
(more than 16 long segments, more than 1,024 pending ranges, scans of more
than 512 and 256 entries) are asserted on the model's record."""
import numpy as np
import pytest

import fold_cases as fc
from oracle_lib import Oracle, assert_states_equal

NAMES = [n for n, _, _ in fc.FAMILIES]
PATHS = ("group", "long")


def _matrix():
    m = set()
    # A: segment shape and placement
    m |= {"A.len0.empty", "A.len1.group", "A.len7.group", "A.len8.group", "A.len9.long", "A.len63.long",
          "A.len64.long", "A.len65.long", "A.len128.long", "A.len129.long", "A.empty_between",
          "A.null_seg_begin", "A.uncovered_head", "A.uncovered_tail", "A.all_live"}
    m |= {f"A.nseg{n}" for n in (1, 7, 8, 9, 15, 16, 17)}
    m |= {f"A.waves{w}" for w in (1, 2, 7, 8, 9, 15, 16, 17, 25)}
    m |= {f"A.long_at{p}" for p in range(8)} | {"A.wave_long2", "A.wave_long8", "A.long_gt16", "A.pending_gt1024"}
    # B: rejections beside a segment of the same wave that folds
    for why in ("other_slot", "peer_neg", "peer_ge_P", "peer_me"):
        m |= {f"B.{why}.group.klast", f"B.{why}.long.k63", f"B.{why}.long.k64", f"B.{why}.long.klast"}
        if why != "other_slot":     # record 0's slot is the segment's
            m |= {f"B.{why}.group.k0", f"B.{why}.long.k0"}
    for p in PATHS:
        m |= {f"B.n_neg.{p}.k0", f"B.n_neg.{p}.klast", f"B.idx_top.{p}.k0", f"B.idx_top.{p}.klast",
              f"B.idx_top_ok.{p}", f"B.first_slot_oob.{p}", f"B.bad_state.{p}", f"B.rejected_stepdown.{p}"}
    m |= {"B.dup.same_wave", "B.dup.other_wave", "B.dup.of_rejected", "B.dup.group_beats_long",
          "B.dup.long_beats_group", "B.P1"}
    # C: a2
    for p in PATHS:
        m |= {f"C.stepdown.{w}.{p}" for w in ("first", "middle", "last")}
        m |= {f"C.{k}.{p}" for k in ("ignored_success_after_stepdown", "stale_reply", "args_term", "prev_mismatch",
                                     "success", "fail", "need_more.set_at_last", "need_more.clear_at_last1",
                                     "repeat.prev_updated", "repeat.stale_prev", "match_down", "nothing_applied")}
        m |= {f"C.nonleader_{k}.{r}.{p}" for k in ("stepdown", "ignored") for r in ("follower", "candidate")}
    m |= {"C.stepdown.k63.long", "C.stepdown.k64.long"}
    # D: the order statistic
    for P in range(2, 9):
        m |= {f"D.P{P}.{k}" for k in ("self_high", "self_low", "clipped", "no_range", "no_range.group", "no_range.long")}
        if P >= 3:
            m |= {f"D.P{P}.tie", f"D.P{P}.tie.group", f"D.P{P}.tie.long"}
    # E: ranges and both scans
    for p, vals in (("group", fc.SCAN_GROUP), ("long", fc.SCAN_LONG)):
        E = f"E.{p}."
        m |= {E + k for k in ("len1_hit", "len1_miss", "probe_hit", "settled", "sorted_top_above.scan_hit",
                              "unsorted_top_below.scan", "hit_hi1", "term_at_commit", "term_below_commit",
                              "commit_eq_dummy", "wraps", "ranges2", "ranges3", "multi.probehit_scanmiss",
                              "multi.scanmiss_probehit", "multi.probehit_scanhit", "multi.scanhit_scanhit", "term_max",
                              "index_top")}
        m |= {E + "ring0." + r for r in fc.RING0}
        m |= {E + f"d{v}.hit" for v in vals}
        m |= {E + f"n{v}.{k}" for v in vals if v for k in ("hit_lo", "miss")}
        m |= {f"E.iter2.{p}", f"E.upper_vectors.{p}"}
    m |= {"E.group.multi.scanhit_scanhit.two_waves", "E.long.batch1.scan"}
    return m


MATRIX = _matrix()
# cells that come with a family's shape and are claimed beside the matrix
INCIDENTAL = {"A.nseg20", "A.waves3", "A.waves138"} | {f"A.nseg{n}" for n in fc.NSEG}

_runs = {}


def _run(name):
    """(trace, cells) of the family's batch; model == oracle checked on the way."""
    if name in _runs:
        return _runs[name]
    G, P, L, st, items, seg, _ = fc.family(name)
    o = Oracle(G, P, L, st)
    assert np.array_equal(o.state()["terms_sorted"], st["terms_sorted"]), f"{name}: the builder's terms_sorted"
    lp = fc.leader_peers(st, G, P)
    cur = st
    tr0 = None
    for call in range(2):
        if call:
            items, seg = fc.followup(name, o.state(), G, P, L, lp)
        f, err, cur, tr = fc.model_fold(G, P, L, cur, items, seg)
        of, oerr = o.process_append_replies(items, seg)
        assert np.array_equal(err, oerr), f"{name} call {call}: item errors at {np.nonzero(err != oerr)[0][:8]}"
        assert np.array_equal(f, of), f"{name} call {call}: flags at {np.nonzero(f != of)[0][:8]}"
        assert_states_equal(cur, o.state(), G, P, L, f"{name} call {call}: model vs oracle")
        tr0 = tr0 or tr
    _runs[name] = (tr0, fc.cells(tr0))
    return _runs[name]


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle_and_cells_present(name):
    tr, found = _run(name)
    claims = fc.family(name)[6]
    assert claims - found == set(), f"{name}: claimed cells the model does not find"
    if name != "p1":
        assert any(s["n"] and not s["err"] for s in tr["segs"]), f"{name}: nothing folds"


def test_claims_are_the_matrix():
    claimed = set()
    for name in NAMES:
        claimed |= fc.family(name)[6]
    assert MATRIX - claimed == set(), "matrix cells no family claims"
    assert claimed - MATRIX - INCIDENTAL == set(), "claims the matrix does not list"


def test_call_level_claims_default_build():
    """What the shipped grids need to stride: more than 16 long segments and
    more than 1,024 pending ranges in one call; second scan iterations: a
    pending-list scan over more than 512 entries, a long-path scan over more
    than 256, both as a miss over the whole range and as a hit beyond it."""
    assert _run("longpos")[0]["long"] > 16
    assert _run("pending")[0]["pending"] > 1024
    for name in ("scan2048", "scan1541"):
        reps = _run(name)[0]["replies"]
        for path, U in (("group", 512), ("long", 256)):
            scans = [R for R in reps if R["path"] == path and R["cls"] in ("scanhit", "scanmiss")]
            assert max(R["rng"][1] - R["rng"][0] for R in scans if R["cls"] == "scanmiss") > U
            assert max(R["d"] for R in scans if R["cls"] == "scanhit") >= U
            # a third iteration too
            assert max(R["d"] for R in scans if R["cls"] == "scanhit") >= 2 * U
        # capacity not a multiple of four in one of the two
    assert fc.family("scan1541")[2] % 4 != 0 and fc.family("scan2048")[2] == 2048


def test_every_a_segment_is_live():
    """In the A families every non-empty segment holds a reply with a non-zero
    flag or error in the oracle's answer: a skipped or twice-folded segment shows."""
    for name in ["lengths", "null", "uncovered", "longpos", "pending"] + [f"nseg{n}" for n in fc.NSEG]:
        G, P, L, st, items, seg, _ = fc.family(name)
        f, err = Oracle(G, P, L, st).process_append_replies(items, seg)
        sb = np.arange(len(items) + 1) if seg is None else seg
        for b, e in zip(sb[:-1], sb[1:]):
            assert b == e or (f[b:e] != 0).any() or (err[b:e] != 0).any(), (name, int(b))
        # ... and the items no segment covers stay 0 / 0
        assert not f[:sb[0]].any() and not err[:sb[0]].any() and not f[sb[-1]:].any() and not err[sb[-1]:].any()


def test_rejected_segments_change_no_state():
    """B: a rejected segment, a step-down reply in it or not, leaves its replica as it was."""
    G, P, L, st, items, seg, _ = fc.family("reject")
    o = Oracle(G, P, L, st)
    f, err = o.process_append_replies(items, seg)
    after = o.state()
    gp = G * P
    for b, e in zip(seg[:-1], seg[1:]):
        s = int(items["slot"][b])
        if err[b] and 0 <= s < gp and err[b] != fc.ITEM_DUP_SLOT:
            assert (f[b:e] == 0).all()
            for k in ("current_term", "state", "commit_index", "voted_for"):
                assert after[k][s] == st[k][s], (k, s)
            assert np.array_equal(after["match_index"][s * P:(s + 1) * P], st["match_index"][s * P:(s + 1) * P])
            assert np.array_equal(after["next_index"][s * P:(s + 1) * P], st["next_index"][s * P:(s + 1) * P])
