"""CPU checks of the in-place crash's cases and model (tests/crash_cases.py,
tests/crash_model.py): the feature's constants, every cell the case families
claim, every batch and every schedule on the model alone. No GPU."""
import numpy as np
import pytest

import crash_cases as cc
from crash_model import CrashModel
from oracle_lib import logical_logs
from snapshot_matrix_cases import ROW_LENS, WRAPS

from multiraft_amd import Engine, _abi, features
from multiraft_amd._abi import CANDIDATE, FOLLOWER, ITEM_BAD_SLOT, ITEM_BAD_STATE, LEADER


def test_feature_bit_and_constants():
    assert _abi.FEATURE_CRASH == 4 and features() & _abi.FEATURE_CRASH
    assert _abi.TIMER_NEVER == 2**31 - 1 > 1 << 30          # no `now` (<= 2^30) reaches it
    assert "mraft_crash" in _abi.ABI_SYMBOLS and callable(Engine.crash)
    assert _abi.lib().mraft_abi_version() == 6


# ---- R --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,L", cc.R_SHAPES)
def test_r_family_holds_every_cell(P, L):
    fam = cc.family(f"R{P}_{L}")
    st, G = fam["st"], fam["G"]
    gp = G * P
    assert G <= 64
    n = st["last_index"] - st["dummy_index"]
    me = np.arange(gp) % P
    cells = {
        "leader": st["state"] == LEADER, "candidate": st["state"] == CANDIDATE, "follower": st["state"] == FOLLOWER,
        "commit above dummy": st["commit_index"] > st["dummy_index"],
        "applied below commit": st["last_applied"] < st["commit_index"],
        "has_snapshot": st["has_snapshot"] == 1,
        **{f"persist {b}": st["persist_dirty"] == b for b in range(4)},
        "votes": st["granted_votes"] > 0,
        "match row": st["match_index"].reshape(gp, P).any(axis=1),
        "next row": st["next_index"].reshape(gp, P).any(axis=1),
        "voted -1": st["voted_for"] == -1, "voted me": st["voted_for"] == me, "voted junk": st["voted_for"] == P,
        "head 0": (st["log_head"] == 0) & (n > 0), "head mid": (st["log_head"] == L // 2) & (n > 0),
        "head L-1": (st["log_head"] == L - 1) & (n > 0),
        "dummy 0": st["dummy_index"] == 0, "dummy > 0": st["dummy_index"] > 0,
        "empty log": n == 0, "full ring": n == L - 1,
        "wrapped log": st["log_head"] + n >= L,
        "no proof": st["terms_sorted"] == 0,
        "as Make left it": (st["current_term"] == 0) & (n == 0) & (st["voted_for"] == -1),
    }
    if P > 1:
        cells["voted other"] = (st["voted_for"] >= 0) & (st["voted_for"] < P) & (st["voted_for"] != me)
    crashed = np.zeros(gp, bool)
    for slots, _ in fam["batches"]:
        crashed[slots[(slots >= 0) & (slots < gp)]] = True
    for name, where in cells.items():
        assert (where & crashed).any(), (P, L, name, "no crashed replica holds this cell")
    assert [len(s) for s, _ in fam["batches"]] == [0, 1, 4, 5, 63, 64, 65, 257]
    assert sorted(len(s) for s, null in fam["batches"] if null) == list(cc.NULL_ERR_SIZES)
    for slots, _ in fam["batches"]:
        if len(slots) >= 4:
            assert slots[1] == -1 and slots[2] == gp and slots[3] == slots[0]
        named = np.unique(slots[(slots >= 0) & (slots < gp)])
        assert len(named) < gp or len(slots) > gp, "some replica is not named"
    big = fam["batches"][-1][0]
    assert len(big) == 257 and (P > 4 or len(np.unique(big)) < len(big) - 2)    # repeats beyond item 3's


# ---- T --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", cc.T_LS)
def test_t_family_holds_every_cell(L):
    fam = cc.family(f"T{L}")
    st, G, P = fam["st"], fam["G"], fam["P"]
    rows, slots = fam["rows"], set(fam["batches"][0][0].tolist())
    assert {r[0] for r in rows} == set(ROW_LENS) | {L - 1} and {r[1] for r in rows} == set(WRAPS)
    logs = logical_logs(st, G, P, L).astype(np.int64)
    seen = {("descent", d): 0 for d in cc.T_DESCENTS}
    seen.update({"withheld": 0, "kept": 0, "wraps": set(), "lens": set(), "not named": 0})
    for s, (n, w, kind, d) in enumerate(rows):
        assert st["last_index"][s] - st["dummy_index"][s] == n
        assert st["log_head"][s] == (L - w) % L             # entry w at ring position 0
        t = logs[s, :n + 1]
        desc = np.nonzero(t[1:-1] > t[2:])[0] + 1            # descents after the dummy: (i, i + 1)
        if kind == "descent" and d != (0, 1):
            assert desc.tolist() == [d[0]] and fam["expect"][s] == 0 and fam["srt"][s] == 0
        else:
            assert not len(desc) and fam["expect"][s] == 1
            assert fam["srt"][s] == (1 if kind == "kept" else 0)
        if kind == "descent" and d == (0, 1):
            assert t[0] > t[1]
        if s not in slots:
            seen["not named"] += 1
            continue
        seen[("descent", d) if kind == "descent" else kind] += 1
        seen["wraps"].add(w)
        seen["lens"].add(n)
    assert seen["wraps"] == set(WRAPS) and seen["lens"] == set(ROW_LENS) | {L - 1}
    assert all(v > 0 for k, v in seen.items() if not isinstance(v, set)), seen


# ---- B --------------------------------------------------------------------------------------------
def test_b_family_is_broken_where_it_says():
    fam = cc.family("B")
    st, L = fam["st"], fam["L"]
    n = st["last_index"].astype(np.int64) - st["dummy_index"]
    assert n[1] < 0 and n[4] == L and ((n >= 0) & (n < L)).sum() == len(n) - 2
    assert (fam["expect_err"] != 0).sum() == 2 and (fam["expect_err"][[1, 4]] == ITEM_BAD_STATE).all()


# ---- every batch on the model ------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_family_on_the_model(name):
    assert cc.run_family_model(name) == cc.n_items(name)


def test_model_errors_and_duplicates():
    fam = cc.family("R3_16")
    G, P, L = fam["G"], fam["P"], fam["L"]
    m = CrashModel(G, P, L, fam["st"])
    err = m.crash(np.array([5, -1, G * P, 5, 2**31 - 1, -2**31], np.int64))
    assert err.tolist() == [0, ITEM_BAD_SLOT, ITEM_BAD_SLOT, 0, ITEM_BAD_SLOT, ITEM_BAD_SLOT]
    once = CrashModel(G, P, L, fam["st"])
    once.crash([5])
    for k, v in m.state().items():
        assert np.array_equal(v, once.state()[k]), k
    assert m.ed is None                                      # no timers: the state part only
    m.enable(1, 3, 10, 30, 0)
    m.crash([7, 8])
    assert (m.ed[[7, 8]] == _abi.TIMER_NEVER).all() and (m.hd[[7, 8]] == _abi.TIMER_NEVER).all()
    assert (m.ed[:7] < 31).all()
    assert len(m.crash(np.zeros(0, np.int32))) == 0


# ---- the schedules -----------------------------------------------------------------------------------
def test_schedules_are_the_reference_s():
    P, sched = cc.SCENARIOS["Persist1"]
    full = (1 << P) - 1
    assert sched[1][0](P, 1, 0, full) == ("bounce", full)
    assert sched[2][0](P, 1, 0, full) == (0b101, full)
    assert sched[4][0](P, 2, 0, full) == (0b010, full)       # the leader and leader + 1: no quorum
    P, sched = cc.SCENARIOS["Persist2"]
    full = (1 << P) - 1
    ups = [full]
    for fn, _ in sched[1:]:
        ups.append(fn(P, 0, 0, ups[-1])[0])
    assert ups == [0b11111, 0b11001, 0b00110, 0b01110, 0b11111]
    P, sched = cc.SCENARIOS["Persist3"]
    assert sched[1][0](P, 0, 0, 0b111) == (0b111, 0b011)     # leader + 2 cut off
    assert sched[2][0](P, 0, 0, 0b111) == (0b100, 0b111)     # leader and leader + 1 crash, leader + 2 reconnects
    assert sched[3][0](P, 0, 0, 0b100) == (0b101, 0b111)
    P = 5
    up, seen = 0b11111, []
    for L in (0, 1, 2, 3, 4):                                # Figure8: the Leader crashes every phase
        up, _ = cc._figure8(P, L, 0, up)
        seen.append(up)
        assert not up >> L & 1 and bin(up).count("1") >= 3
    assert seen[:3] == [0b11110, 0b11100, 0b11001]           # fewer than a majority up: one restarts


@pytest.mark.parametrize("P", (3, 5))
def test_scenarios_on_the_model(P):
    """Every schedule on CrashModel alone: the liveness bound is a condition on
    the model (the timeout range and seed are reach_cases.SCEN_CFG's, unchanged)."""
    c = cc.run_scenarios(P, 64)
    assert c["majority_leader"] > 64 and c["agree"] > 64 and c["no_quorum"] > 0, c
    assert c["crashes"] > 64 and c["restarts"] > 64 and c["leader_crashed"] > 32 and c["down_ticks"] > 1000, c
    assert c["reapplied"] > 64 and c["elected_after_crash"] > 0, c
    if P == 3:
        assert c["bounce"] > 0, c
