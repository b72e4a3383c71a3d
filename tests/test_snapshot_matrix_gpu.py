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
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import snapshot_matrix_cases as mc
from oracle_lib import Oracle, assert_states_equal

from multiraft_amd import DEVICE, Engine, _abi
from multiraft_amd._abi import IS_ARGS, IS_RESULT, ITEM_NEED_SNAPSHOT

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


def _i32(t, a, dev):
    return t.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(len(a), -1).copy()).to(dev)


@pytest.mark.parametrize("name", ["snapshot_big", "handle5_13", "fold5_13"])
def test_device_buffers_back_to_back_gpu(name):
    """MRAFT_DEVICE batch buffers: the family's batch and its follow-up
    enqueued back to back behind a device spin, no host wait between them."""
    import torch
    G, P, L, st, b, _ = mc.family(name)
    kind = mc.KIND[name]
    o = Oracle(G, P, L, st)
    dev = torch.device("cuda", 0)
    lib = _abi.lib()
    fill = lambda n: torch.full((n,), -1, dtype=torch.int32, device=dev)  # noqa: E731
    calls, want, outs = [], [], []
    if kind == "snapshot":
        for sl, ix in ((b["slots"], b["index"]), mc.followup_snapshot(b)):
            want.append([o.snapshot(sl, ix)])
            bufs = (_i32(torch, sl, dev), _i32(torch, ix, dev), fill(len(sl)))
            outs.append(bufs[2:])
            calls.append(lambda h, q=bufs, n=len(sl): lib.mraft_snapshot(h, q[0].data_ptr(), q[1].data_ptr(), n,
                                                                         q[2].data_ptr(), DEVICE))
    elif kind == "handle":
        for a in (b["args"], mc.followup_handle(b)):
            rep, fl, err = o.handle_install_snapshot(a)
            want.append([rep.view(np.int32), fl, err])
            n = len(a)
            bufs = (_i32(torch, np.ascontiguousarray(a, IS_ARGS), dev), fill(2 * n), fill(n), fill(n))
            outs.append(bufs[1:])
            calls.append(lambda h, q=bufs, n=n: lib.mraft_handle_install_snapshot(
                h, q[0].data_ptr(), n, q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), DEVICE))
    else:
        for it, sg in ((b["items"], b["seg"]), mc.followup_fold(b)):
            want.append(list(o.process_install_snapshot_replies(it, sg)))
            n = len(it)
            bufs = (_i32(torch, np.ascontiguousarray(it, IS_RESULT), dev),
                    torch.from_numpy(np.ascontiguousarray(sg, np.int64)).to(dev), fill(n), fill(n))
            outs.append(bufs[2:])
            calls.append(lambda h, q=bufs, n=n, ns=len(sg) - 1: lib.mraft_process_install_snapshot_replies(
                h, q[0].data_ptr(), n, q[1].data_ptr(), ns, q[2].data_ptr(), q[3].data_ptr(), DEVICE))
    with Engine(G, P, L) as e:
        e.load_state(st)
        stream = torch.cuda.ExternalStream(e.stream(), device=dev)
        e.synchronize()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(1e8))  # device spin ahead of the calls
        for call in calls:
            assert call(e._h) == 0, _abi.last_error()
        assert not stream.query(), "a call waited on the device"
        e.synchronize()
        got = e.store_state()
    for k, (w, g) in enumerate(zip(want, outs)):
        for j, (a, t) in enumerate(zip(w, g)):
            assert np.array_equal(t.cpu().numpy().reshape(-1), np.asarray(a).reshape(-1)), (name, k, j)
    assert_states_equal(got, o.state(), G, P, L, f"{name}: two device calls back to back")


def test_small_grid_library_child_gpu():
    """Every family in a fresh process on the small-grid library: all ok, and
    the whole list ran."""
    assert os.path.exists(GRID1), "build() makes the small-grid library"
    env = dict(os.environ, MRAFT_LIB=GRID1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "snapshot_matrix_cases.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.stdout.strip(), r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert [c[0] for c in out["cases"]] == mc.NAMES, out["cases"]
    assert all(c[2] is True and c[1] == (mc.n_items(c[0]) if mc.KIND[c[0]] != "cross" else
                                         mc.family(c[0])[0] * mc.family(c[0])[1])
               for c in out["cases"]), (out["cases"], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
