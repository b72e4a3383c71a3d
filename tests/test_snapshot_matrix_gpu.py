"""The directed cases of the item-level kernels (tests/snapshot_matrix_cases.py;
their cells are proved present by tests/test_snapshot_matrix.py) on
libmraft_hip.so against the CPU oracle, bit for bit: every output of the
family's script (outputs, item errors, flags, read-out headers and terms,
persist bits, group flags of the tick) and the whole state with ring heads,
after the family's batch and after a follow-up batch on the same engine (the
claim epoch reused); the cross-path groups through the message-level calls and
through mraft_replicate_tick in every mode; a snapshot, a handle and a fold
family with device-resident batch buffers, two calls back to back without a
host wait; and every family in a child process on the small-grid library
(multiraft_amd/libmraft_hip_grid1.so: the strided grids of this unit at one
workgroup, so the stride loops of k_init_state, k_collect_apply,
k_collect_persist and k_terms_sorted run their later passes)."""
import os

import numpy as np
import pytest

import snapshot_matrix_cases as mc
from gpu_support import behind_spin, run_cases_child
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import DEVICE, Engine
from multiraft_amd._abi import IS_ARGS, IS_RESULT, ITEM_NEED_SNAPSHOT, from_words, to_words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID1 = os.path.join(ROOT, "multiraft_amd", "libmraft_hip_grid1.so")


@pytest.mark.parametrize("name", mc.NAMES)
def test_family_gpu(name):
    mc.run_family(name, Engine, Oracle, assert_states_equal)


@pytest.mark.parametrize("name", [n for n in mc.NAMES if mc.KIND[n] == "gather"])
def test_need_snapshot_exactly_where_args_gpu(name):
    G, P, L, st, b, _ = mc.family(name)
    with Engine(G, P, L) as e:
        e.load_state(st)
        ia, ierr = e.gather_install_snapshot_args(b["slots"], b["peers"])
        _, aerr = e.gather_append_args(b["slots"], b["peers"])
    made = (ierr == 0) & (ia["slot"] >= 0)
    assert np.array_equal(made, aerr == ITEM_NEED_SNAPSHOT) and made.any() and (~made & (ierr == 0)).any()


@pytest.mark.parametrize("name", ["snapshot_big", "handle5_13", "fold5_13"])
def test_device_buffers_back_to_back_gpu(name):
    """MRAFT_DEVICE batch buffers: the family's batch and its follow-up
    enqueued back to back behind a device spin, no host wait between them."""
    import torch
    G, P, L, st, b, _ = mc.family(name)
    kind = mc.KIND[name]
    o = Oracle(G, P, L, st)
    dev = torch.device("cuda", 0)
    fill = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)  # noqa: E731
    plain = lambda a, dt=np.int32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    calls, want, outs = [], [], []       # per call: the enqueue, the oracle's outputs, the device buffers
    if kind == "snapshot":
        for sl, ix in ((b["slots"], b["index"]), mc.followup_snapshot(b)):
            want.append([o.snapshot(sl, ix)])
            outs.append((fill(len(sl)),))
            calls.append(lambda e, q=(plain(sl), plain(ix)), out=outs[-1]: e.snapshot(*q, where=DEVICE, out=out))
    elif kind == "handle":
        for a in (b["args"], mc.followup_handle(b)):
            want.append(list(o.handle_install_snapshot(a)))
            outs.append((fill(len(a), 2), fill(len(a)), fill(len(a))))
            calls.append(lambda e, q=to_words(np.asarray(a, IS_ARGS), dev), out=outs[-1]:
                         e.handle_install_snapshot(q, where=DEVICE, out=out))
    else:
        for it, sg in ((b["items"], b["seg"]), mc.followup_fold(b)):
            want.append(list(o.process_install_snapshot_replies(it, sg)))
            outs.append((fill(len(it)), fill(len(it))))
            calls.append(lambda e, q=(to_words(np.asarray(it, IS_RESULT), dev), plain(sg, np.int64)), out=outs[-1]:
                         e.process_install_snapshot_replies(*q, where=DEVICE, out=out))
    with Engine(G, P, L) as e:
        e.load_state(st)
        with behind_spin(e):
            for call in calls:
                call(e)
        got = e.store_state()
    for k, (w, g) in enumerate(zip(want, outs)):
        for j, (a, t) in enumerate(zip(w, g)):
            assert np.array_equal(from_words(t, a.dtype), a), (name, k, j)
    assert_states_equal(got, o.state(), G, P, L, f"{name}: two device calls back to back")


def test_small_grid_library_child_gpu():
    """Every family in a fresh process on the small-grid library: all ok, and
    the whole list ran."""
    out = run_cases_child(os.path.join(ROOT, "tests", "snapshot_matrix_cases.py"), GRID1)
    assert [c[0] for c in out["cases"]] == mc.NAMES, out["cases"]
    assert all(c[2] is True and c[1] == (mc.n_items(c[0]) if mc.KIND[c[0]] != "cross" else
                                         mc.family(c[0])[0] * mc.family(c[0])[1])
               for c in out["cases"]), out["cases"]
