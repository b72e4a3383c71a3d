"""The assumptions of multiraft_amd/_calls.py, checked without a GPU: the two
libraries' C signatures have the shape the shared bodies pass (nothing else
ties the oracle's signatures to the product's), the record <-> word-tensor
conversions of `_abi` are exact inverses for every record dtype, and `out=` /
`where` behave as stated on the oracle."""
import ctypes

import numpy as np
import pytest

import oracle_lib
from oracle_lib import Oracle

from multiraft_amd import DEVICE, _abi, new_state
from multiraft_amd._calls import BatchCalls

METHODS = [n for n, f in vars(BatchCalls).items() if callable(f) and not n.startswith("_")]
# the calls that take host arrays only: no trailing `where` in include/mraft.h
NO_WHERE = {"read_persistent", "restore"}
RECORDS = {n: v for n, v in vars(_abi).items() if isinstance(v, np.dtype) and v.fields}


def test_every_batched_call_is_covered():
    assert len(METHODS) == 15 and NO_WHERE <= set(METHODS), METHODS


@pytest.mark.parametrize("name", METHODS + ["handle_append_entries"])
def test_signatures_have_the_shared_shape(name):
    """mraft_<name>(handle, X..., where) and ora_<name>(engine, X...)."""
    res, args = _abi._SIGS["mraft_" + name]
    tail = [] if name in NO_WHERE else [ctypes.c_int32]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p] + oracle_lib.SIGS["ora_" + name][1:] + tail, name
    assert oracle_lib.SIGS["ora_" + name][0] is oracle_lib._E


@pytest.mark.parametrize("name", sorted(RECORDS))
@pytest.mark.parametrize("n", [0, 1, 7])
def test_record_conversions_round_trip(name, n):
    import torch
    dt = RECORDS[name]
    assert dt.itemsize % 4 == 0
    rng = np.random.default_rng(len(name) + n)
    raw = rng.integers(0, 256, size=2 * n * dt.itemsize, dtype=np.uint8)
    recs = raw.view(dt)[::2]                      # every byte random (padding too), not contiguous
    words = _abi.to_words(recs)
    assert words.dtype == torch.int32 and tuple(words.shape) == (n, dt.itemsize // 4) and words.is_contiguous()
    assert words.numpy().tobytes() == np.ascontiguousarray(recs).tobytes()
    back = _abi.from_words(words, dt)
    assert back.dtype == dt and back.shape == (n,) and back.tobytes() == np.ascontiguousarray(recs).tobytes()
    words[:] = 0                                   # a copy: the records are untouched
    assert np.ascontiguousarray(recs).tobytes() == raw.view(dt)[::2].tobytes()


def test_the_sizes_the_issue_names():
    assert RECORDS["AE_ARGS"].itemsize == 40 and RECORDS["PERSISTENT"].itemsize == 32
    assert {"AE_ARGS", "AE_REPLY", "AE_RESULT", "RV_ARGS", "RV_REPLY", "RV_RESULT", "IS_ARGS", "IS_REPLY", "IS_RESULT",
            "PERSISTENT"} == set(RECORDS)


def _leaders(G, P, L):
    st = new_state(G, P, L)
    st["state"][::P] = _abi.LEADER
    st["current_term"][:] = 3
    return st


def test_out_buffers_are_filled_and_returned():
    G, P, L = 4, 3, 8
    slots = np.arange(G, dtype=np.int32) * P
    a, b = Oracle(G, P, L, _leaders(G, P, L)), Oracle(G, P, L, _leaders(G, P, L))
    want = a.start(slots, None)
    out = tuple(np.full(G, -1, np.int32) for _ in range(4))
    got = b.start(slots, None, out=out)
    assert all(g is o for g, o in zip(got, out))
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and (want[2] == 1).all()
    persist = np.full(G * P, -1, np.int32)
    assert b.collect_persist(out=(persist,)) is persist and np.array_equal(persist, a.collect_persist())
    fr, to = np.full(G * P, -1, np.int32), np.full(G * P, -1, np.int32)
    assert b.collect_apply(out=(fr, to, None, None)) == (fr, to)
    assert all(np.array_equal(g, w) for g, w in zip((fr, to), a.collect_apply()))


def test_the_oracle_refuses_device_mode():
    G, P, L = 2, 3, 8
    o = Oracle(G, P, L, _leaders(G, P, L))
    before = o.store_state()
    with pytest.raises(ValueError):
        o.start(np.zeros(1, np.int32), None, where=DEVICE, out=tuple(np.zeros(1, np.int32) for _ in range(4)))
    with pytest.raises(ValueError):
        o.collect_persist(where=DEVICE)            # no input to take a device from, and no out=
    assert all(np.array_equal(v, before[k]) for k, v in o.store_state().items())
