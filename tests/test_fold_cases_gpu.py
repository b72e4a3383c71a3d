"""The directed cases of the reply fold (tests/fold_cases.py; their cells are
proved present by tests/test_fold_cases.py) on libmraft_hip.so against the CPU
oracle, bit for bit: flags, item errors and the whole state after the family's
batch and after a follow-up batch on the same engine (the claim epoch reused,
the list counters zeroed again); the scan families with terms_sorted withheld
(the same decisions by Go's scans alone); a structural and a scan family with
device-resident batch buffers, two calls back to back without a host wait; and
every family in a child process on the small-grid library
(multiraft_amd/libmraft_hip_grid1.so: the fold's three grids at one workgroup,
so k_fold's stride loop and both loops of k_fold_tail run)."""
import os

import numpy as np
import pytest

import fold_cases as fc
from gpu_support import behind_spin, run_cases_child
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import DEVICE, Engine
from multiraft_amd._abi import AE_RESULT, to_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID1 = os.path.join(ROOT, "multiraft_amd", "libmraft_hip_grid1.so")
NAMES = [n for n, _, _ in fc.FAMILIES]


@pytest.mark.parametrize("name", NAMES)
def test_family_gpu(name):
    fc.run_family(name, Engine, Oracle, assert_states_equal)


@pytest.mark.parametrize("name", fc.SCAN_FAMILIES)
def test_scan_family_without_the_proof_gpu(name):
    """terms_sorted all 0 (bound as is, mraft_bind_state): nothing settles,
    every open range is scanned, and the decisions are the oracle's."""
    import torch
    G, P, L, st, items, seg, _ = fc.family(name)
    lp = fc.leader_peers(st, G, P)
    dev = torch.device("cuda", 0)
    d = {k: torch.from_numpy(v.copy()).to(dev) for k, v in st.items()}
    d["terms_sorted"].fill_(0)
    o = Oracle(G, P, L, st)
    with Engine(G, P, L, alloc=False) as e:
        e.bind(d)
        for call in range(2):
            if call:
                items, seg = fc.followup(name, o.state(), G, P, L, lp)
            f, err = e.process_append_replies(items, seg)
            of, oerr = o.process_append_replies(items, seg)
            assert np.array_equal(err, oerr) and np.array_equal(f, of), (name, call)
            got = {k: v.cpu().numpy() for k, v in d.items()}
            want = dict(o.state())
            assert not got.pop("terms_sorted").any()
            want.pop("terms_sorted")
            assert_states_equal(got, want, G, P, L, f"{name} call {call}, proof withheld")


@pytest.mark.parametrize("name", ["longpos", "scan2048"])
def test_device_buffers_back_to_back_gpu(name):
    """MRAFT_DEVICE batch buffers: the family's batch and its follow-up
    enqueued back to back behind a device spin, no host wait between them."""
    import torch
    G, P, L, st, items, seg, _ = fc.family(name)
    o = Oracle(G, P, L, st)
    want = [o.process_append_replies(items, seg)]
    batches = [(items, seg), fc.followup(name, o.state(), G, P, L, fc.leader_peers(st, G, P))]
    want.append(o.process_append_replies(*batches[1]))
    dev = torch.device("cuda", 0)
    fill = lambda n: torch.full((n,), -1, dtype=torch.int32, device=dev)  # noqa: E731
    bufs = [(to_words(np.asarray(it, AE_RESULT), dev), torch.from_numpy(np.ascontiguousarray(sg, np.int64)).to(dev),
             fill(len(it)), fill(len(it))) for it, sg in batches]
    with Engine(G, P, L) as e:
        e.load_state(st)
        with behind_spin(e, what="a fold call"):
            for it_d, sg_d, fl_d, err_d in bufs:
                e.process_append_replies(it_d, sg_d, where=DEVICE, out=(fl_d, err_d))
        got = e.store_state()
    for k, ((of, oerr), (_, _, fl_d, err_d)) in enumerate(zip(want, bufs)):
        assert np.array_equal(err_d.cpu().numpy(), oerr) and np.array_equal(fl_d.cpu().numpy(), of), (name, k)
    assert_states_equal(got, o.state(), G, P, L, f"{name}: two device calls back to back")


def test_small_grid_library_child_gpu():
    """Every family in a fresh process on the small-grid library: all ok, and
    the whole list ran."""
    out = run_cases_child(os.path.join(ROOT, "tests", "fold_cases.py"), GRID1)
    assert [c[0] for c in out["cases"]] == NAMES, out["cases"]
    assert all(c[2] is True and c[1] == len(fc.family(c[0])[4]) for c in out["cases"]), out["cases"]
