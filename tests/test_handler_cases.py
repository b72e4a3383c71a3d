"""The directed cases of the AppendEntries handler (tests/handler_cases.py) on
the CPU, before any GPU sees them.

Per family: the plain Python model equals the C oracle on replies, item
errors, the _ex records and the whole state (persist bits included) after
every call of the script and after its follow-up batch; the builder's
terms_sorted is the oracle's; every input keeps the oracle inside its domain;
and every cell the family claims is found by `handler_cases.cells`, which sees
only `geometry` (from the args alone) and the model's per-item record, under
the stage capacities the family runs with: a cell taken out of a builder fails
here by name. MATRIX lists the cells one by one; the families' claims together
must be exactly that set, none omitted."""
import numpy as np
import pytest

import handler_cases as hc
from oracle_lib import Oracle, assert_states_equal


def _matrix():
    m = set()
    for ni in range(1, 8):
        m |= {f"K.run.ni{ni}.len{ln}" for ln in {1, ni - 1, ni, ni + 1, 2 * ni, 2 * ni + 1} - {0}}
    m |= {f"K.edge.{off:+d}" for off in range(-7, 8)}
    m |= {f"K.n{n}" for n in (1, 63, 64, 65, 129)} | {f"K.n{n}" for n in range(1, 10)} | {"K.end_in_run"}
    m |= {f"K.head_lane{q}" for q in range(7)} | {"K.cross_window", "K.window_all_heads"}
    m |= {f"K.waves{w}" for w in (1, 7, 8, 9, 15, 16, 17, 25)}
    m |= {"K.near.row", "K.near.base", "K.near.end"}
    m |= {f"K.mask.{k}.{p}" for k in hc.MASK_KINDS for p in ("head", "middle", "last")}
    m |= {"K.idx_top_ok", "K.first_merge.lane0", "K.first_merge.lane1", "K.first_merge.laneLast", "K.nobody_merges",
          "K.hb_set", "K.hb_heads_set", "K.hb_full.mid", "K.hb_full.last", "K.hb_past.1", "K.hb_past.5L"}
    m |= {"V." + k for k in hc.V_CLASSES} | {"V.exact_end", "V.one_over", "V.hb_past", "V.empty_buffer"}
    m |= {"D.written_by.normal", "D.written_by.dup", "D.not_written_by.idx_bad", "D.not_written_by.heartbeat",
          "D.not_written_by.ref_bad", "D.staged_claimant.deferred", "D.staged_claimant.ref_bad",
          "D.staged_claimant.idx_bad", "D.self_rewrite", "D.src_wrap.first", "D.src_wrap.middle", "D.src_wrap.last",
          "D.fol_wrap"}
    for cl in hc.D_CLASSES + ("mismatch_scan65wrap",):
        # a heartbeat reads nothing: it is never staged and never on a cycle
        m |= {f"D.cls.{cl}.{p}" for p in (("inplace", "chain") if cl == "heartbeat" else
                                          ("inplace", "staged", "chain", "cycbuf"))}
    m |= {f"D.staged_n{n}" for n in hc.SIZES}
    m |= {f"S.cap{c}" for c in (0, 7, 8, 71)}
    m |= {"S.exact_fill", "S.one_over", "S.one_stripe_over_total_below", "S.all_stripes", "S.wave2_later_unfit",
          "S.wave3_later_unfit"}
    m |= {f"F.chain{ln}.{e}" for ln in (1, 2, 3, 40) for e in ("end_unwritten", "end_refbad")}
    m |= {f"F.readers{k}" for k in (1, 2, 3, 70)}
    m |= {f"F.cyc{ln}.{v}" for ln in hc.CYC_LENS for v in hc.cyc_variants(ln)}
    m |= {"F.two_cycles", "F.chain40_into_cyc3"}
    return m


MATRIX = _matrix()
_runs = {}


def _in_domain(fam, args, st):
    """The oracle's domain: int32 arithmetic that cannot overflow, rings that hold their logs."""
    G, P, L = fam["G"], fam["P"], fam["L"]
    prev, k = args["prev_log_index"].astype(np.int64), args["n_entries"].astype(np.int64)
    assert (prev >= 0).all() and (prev + k <= 2**31 - 1).all() and (prev + k >= -2**31).all()
    assert (args["term"] >= 0).all() and (args["term"] < 2**31 - 1).all()
    assert (np.abs(args["entries_offset"]) < 2**40).all()
    live = st["last_index"].astype(np.int64) - st["dummy_index"]
    assert (live >= 0).all() and (live <= L - 1).all() and (st["last_index"] <= hc.TOP).all()
    assert (st["commit_index"] >= st["dummy_index"]).all() and (st["dummy_index"] >= 0).all()
    assert (st["current_term"] >= 0).all() and (st["log_head"] >= 0).all() and (st["log_head"] < L).all()


def _run(name):
    """The cells the model finds in a family; model == oracle checked on the way."""
    if name in _runs:
        return _runs[name]
    fam = hc.family(name)
    G, P, L = fam["G"], fam["P"], fam["L"]
    o = Oracle(G, P, L, fam["st"])
    assert np.array_equal(o.state()["terms_sorted"], fam["st"]["terms_sorted"]), f"{name}: the builder's terms_sorted"
    model = hc.Model(G, P, L, fam["st"])
    found, n_script = set(), sum(1 for s in fam["steps"] if s[0] != "load")
    before = {}

    def on_call(k):
        before[k + 1] = model.store_state()
        recs[k] = model.rec

    recs = {}
    before[0] = model.store_state()
    got = hc.run_script(model, fam, on_call)
    want = hc.oracle_run(name, Oracle)
    hc.compare_runs(got, want, G, P, L, assert_states_equal, f"{name}: model vs oracle")
    k = 0
    for step in hc.steps_of(fam):
        if step[0] == "load":
            before[k] = fam["st"]
            continue
        args = got[k][0]
        _in_domain(fam, args, before[k])
        if k < n_script:            # the follow-up is compared, not classified
            hc.annotate(fam, args, recs[k], before[k])
            if fam.get("by_value"):
                found |= hc.cells(args, None, recs[k], G, P, L, by_value=True, n_ents=len(step[2]))
            else:
                for cap in fam["caps"]:
                    geo = hc.geometry(args, G, P, L, hc.DEFAULT_STAGE if cap is None else cap)
                    found |= hc.cells(args, geo, recs[k], G, P, L, cap=cap)
        k += 1
    assert k == len(got)
    _runs[name] = found
    return found


@pytest.mark.parametrize("name", hc.NAMES)
def test_model_equals_oracle_and_cells_present(name):
    found = _run(name)
    claims = hc.family(name)["claims"]
    assert claims - found == set(), f"{name}: claimed cells the model does not find"


def test_claims_are_the_matrix():
    claimed = set()
    for name in hc.NAMES:
        claimed |= hc.family(name)["claims"]
    assert MATRIX - claimed == set(), "matrix cells no family claims"
    assert claimed - MATRIX == set(), "claims the matrix does not list"


def test_fallback_families_run_on_every_grid():
    """F: every graph family runs at stage 0 on the default deferred grid and
    with MRAFT_DEFER_GRID_MIN 1, 3, 8 and 9; the small-grid library (two cycle
    buffers) runs the same list in tests/test_handler_cases_gpu.py."""
    graph = [n for n in hc.NAMES if n.startswith("cyc") or n in ("chains", "small_batches")]
    assert len(graph) == len(hc.CYC_LENS) + 2
    for name in graph:
        assert set(hc.modes(name)) >= {(0, g) for g in hc.GRID_MINS}, name
    # with two cycle buffers some workgroups of the deferred launch have none
    # wherever more than two deferred items make the grid: every graph family's first call
    for name in graph[:-1]:
        fam = hc.family(name)
        args = next(s[1] for s in fam["steps"] if s[0] == "call")
        assert hc.geometry(args, fam["G"], fam["P"], fam["L"], 0)["nd"] > 2, name


def test_stage_modes_take_the_paths_they_claim():
    """S: the exact fill stages under 71 words and the batch one word larger
    does not; 7 words are none per stripe; the default stage takes both."""
    for name, cap, fb in (("stage_exact", 71, False), ("stage_over", 71, True), ("stage_exact", 7, True),
                          ("stage_exact", 8, True), ("stage_exact", 0, True), ("stage_over", None, False),
                          ("stage_one_stripe", 71, True), ("stage_one_stripe", 1024, False)):
        fam = hc.family(name)
        assert cap in fam["caps"], (name, cap)
        args = next(s[1] for s in fam["steps"] if s[0] == "call")
        geo = hc.geometry(args, fam["G"], fam["P"], fam["L"], hc.DEFAULT_STAGE if cap is None else cap)
        assert geo["fallback"] is fb, (name, cap, geo["staged"])


def test_near_miss_keys_change_a_log():
    """K: read with the set's key in place of its own (any one field of
    same_key dropped), each near-miss item would leave another log."""
    fam = hc.family("near")
    G, P, L = fam["G"], fam["P"], fam["L"]
    args = fam["steps"][1][1]
    geo = hc.geometry(args, G, P, L)
    base = hc.Model(G, P, L, fam["st"])
    base.handle(args, None)
    seen = 0
    for i in range(1, len(args)):
        a, b = geo["items"][i - 1]["key"], geo["items"][i]["key"]
        if geo["items"][i - 1]["pos"] == 2 and a != b and sum(x != y for x, y in zip(a, b)) == 1:
            wrong = args.copy()
            wrong[i]["entries_offset"] = args[i - 1]["entries_offset"]
            wrong[i]["prev_log_index"], wrong[i]["n_entries"] = args[i - 1]["prev_log_index"], args[i - 1]["n_entries"]
            m = hc.Model(G, P, L, fam["st"])
            m.handle(wrong, None)
            s = int(args[i]["slot"])
            row = lambda t: t.st["log_term"][s * L:(s + 1) * L]  # noqa: E731
            assert not np.array_equal(row(m), row(base)) or m.st["last_index"][s] != base.st["last_index"][s], i
            seen += 1
    assert seen == 3
