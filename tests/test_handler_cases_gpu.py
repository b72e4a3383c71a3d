"""The directed cases of the AppendEntries handler (tests/handler_cases.py; their
cells are proved present by tests/test_handler_cases.py) on libmraft_hip.so
against the CPU oracle, bit for bit: replies, item errors, the _ex records and
the whole state after every call of a family's script and after its follow-up
batch on the same engine, under every stage capacity the family names and, for
the fallback's graph families, on the default deferred grid and with
MRAFT_DEFER_GRID_MIN 1, 3, 8 and 9; the stage's boundary through
MRAFT_STAGE_AUTO; K and D families with device-resident buffers, two calls back
to back behind a device spin; and every family under every mode in one child
process each on the small-grid library (libmraft_hip_grid1.so: two cycle
buffers at L = 64, so the deferred launch's other workgroups return before the
count-out) and on the bounds-checking library (libmraft_hip_dbg.so, its three
violation counters at 0)."""
import os

import numpy as np
import pytest

import handler_cases as hc
from gpu_support import behind_spin, run_cases_child
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import DEVICE, Engine
from multiraft_amd._abi import AE_REPLY, AE_RESULT, from_words, to_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID1 = os.path.join(ROOT, "multiraft_amd", "libmraft_hip_grid1.so")
DBG = os.path.join(ROOT, "multiraft_amd", "libmraft_hip_dbg.so")
RUNS = [(n, cap, g) for n in hc.NAMES for cap, g in hc.modes(n)]


@pytest.mark.parametrize("name,cap,gmin", RUNS, ids=[f"{n}-stage{c}-grid{g}" for n, c, g in RUNS])
def test_family_gpu(name, cap, gmin):
    hc.run_family(name, Engine, Oracle, assert_states_equal, cap, gmin)


def _first_call(name):
    fam = hc.family(name)
    return fam, next(s[1] for s in fam["steps"] if s[0] == "call")


def test_stage_auto_grows_only_past_the_exact_fill_gpu():
    """smax <= cap8, seen through MRAFT_STAGE_AUTO: a stripe filled exactly
    publishes no need (the capacity stays), one word more publishes 8 x the
    fullest stripe and the call after it has a stage that holds the batch."""
    exact, a_exact = _first_call("stage_exact")
    over, a_over = _first_call("stage_over")
    G, P, L = exact["G"], exact["P"], exact["L"]
    assert (G, P, L) == (over["G"], over["P"], over["L"])
    with Engine(G, P, L) as e:
        e.set_stage_capacity(71)
        e.set_stage_capacity(-1)     # MRAFT_STAGE_AUTO from 71 words
        for k, (fam, args) in enumerate([(exact, a_exact), (exact, a_exact), (over, a_over), (over, a_over)]):
            e.load_state(fam["st"])
            o = Oracle(G, P, L, fam["st"])
            rep, err = e.handle_append_entries(args, None)
            orep, oerr = o.handle_append_entries(args, None)
            assert np.array_equal(err, oerr) and np.array_equal(rep, orep), k
            assert_states_equal(e.store_state(), o.state(), G, P, L, f"auto stage, call {k}")
            if k < 3:     # two exact fills, and the overflowing call itself: nothing has grown yet
                assert e.stage_capacity() == 71, (k, e.stage_capacity())
        cap = e.stage_capacity()
        fullest = max(hc.geometry(a_over, G, P, L, 71)["staged"])
        assert fullest == 9 and cap >= 8 * fullest and cap > 71, cap
        assert not hc.geometry(a_over, G, P, L, cap)["fallback"]


@pytest.mark.parametrize("name", hc.DEVICE_FAMILIES)
def test_device_buffers_back_to_back_gpu(name):
    """MRAFT_DEVICE batch buffers: the family's last batch and its follow-up
    enqueued back to back behind a device spin, no host wait between them."""
    import torch
    fam = hc.family(name)
    G, P, L = fam["G"], fam["P"], fam["L"]
    batches = [s[1] for s in hc.steps_of(fam) if s[0] == "call"][-2:]
    o = Oracle(G, P, L, fam["st"])
    want = []
    for a in batches:
        rep, err = o.handle_append_entries(a, None)
        want.append((rep, err, hc.ex_records(a, rep, err, P)))
    dev = torch.device("cuda", 0)
    fill = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)  # noqa: E731
    bufs = [(to_words(a, dev), fill(len(a), 4), fill(len(a), 8), fill(len(a))) for a in batches]
    with Engine(G, P, L) as e:
        e.load_state(fam["st"])
        with behind_spin(e, what="a handler call"):
            for a_d, rep_d, res_d, err_d in bufs:
                e.handle_append_entries(a_d, None, results=True, where=DEVICE, out=(rep_d, res_d, err_d))
        got = e.store_state()
    for k, ((rep, err, res), (_, rep_d, res_d, err_d)) in enumerate(zip(want, bufs)):
        assert np.array_equal(err_d.cpu().numpy(), err), (name, k)
        assert np.array_equal(from_words(rep_d, AE_REPLY), rep), (name, k)
        assert np.array_equal(from_words(res_d, AE_RESULT), res), (name, k)
    assert_states_equal(got, o.state(), G, P, L, f"{name}: two device calls back to back")


def _child(libpath):
    out = run_cases_child(os.path.join(ROOT, "tests", "handler_cases.py"), libpath, drop_env=("MRAFT_DEFER_GRID_MIN",))
    assert [tuple(c[:3]) for c in out["cases"]] == RUNS, "the child ran another list"
    assert all(c[4] is True and c[3] >= 1 for c in out["cases"]), [c for c in out["cases"] if not c[4]]
    return out


def test_small_grid_library_child_gpu():
    """Every family under every mode in a fresh process on the small-grid
    library: at most two workgroups of the deferred launch have a cycle buffer
    (nb < gridDim.x in defer_fallback), all answers the oracle's."""
    _child(GRID1)


def test_bounds_checking_library_child_gpu():
    """The same list on the bounds-checking build: no ring offset out of range."""
    out = _child(DBG)
    assert out["violations"] == {"mraft_debug_bounds_kernels": 0, "mraft_debug_bounds_deferred": 0,
                                 "mraft_debug_bounds_tick": 0}, out["violations"]
