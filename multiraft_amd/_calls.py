"""The batched message-path calls of the boundary (include/mraft.h), each
stated once for the two libraries that export them: libmraft_hip.so
(`mraft_<name>`, engine.Engine) and the CPU oracle (`ora_<name>`,
tests/oracle_lib.Oracle). The two differ in the symbol prefix, the first
argument, the trailing `where` and the error check; a subclass supplies those
in one hook,

    _invoke(name, *c_args, where) -> None     # raises on failure

(where=None: the C call has no such argument), and G, P, L.

Every call takes `where` and `out`:

* where=HOST (the default): inputs are coerced to contiguous arrays of the
  `_abi` dtypes, the call is synchronous and the outputs are numpy arrays.
* where=DEVICE: inputs pass as given (device tensors, or raw device addresses
  with an explicit n=), nothing is coerced and the call only enqueues work on
  the engine's stream.
* out: the call's output buffers in C-argument order (None where the C call
  takes NULL). Absent, they are allocated: zeroed numpy arrays on the host,
  `torch.empty` int32 words ([n, itemsize // 4] for records) on the device of
  the first input. The buffers are passed as they stand, so a prefilled
  item_err reaches the library.
"""
from __future__ import annotations

import numpy as np

from ._abi import (AE_ARGS, AE_RESULT, DEVICE, HOST, IS_ARGS, IS_REPLY, IS_RESULT, PERSISTENT, RV_ARGS,
                   RV_REPLY, RV_RESULT, ptr)

I32 = np.dtype(np.int32)


def _in(a, dtype, where):
    """A host input in its C layout; a device input (or NULL) as given."""
    return a if a is None or where == DEVICE else np.ascontiguousarray(a, dtype=dtype)


def _outs(out, dtypes, n, where, like=None):
    """The caller's output buffers, or fresh ones: one per dtype (None: NULL)."""
    if out is not None:
        return tuple(out)
    dtypes = [None if dt is None else np.dtype(dt) for dt in dtypes]
    if where == HOST:
        return tuple(None if dt is None else np.zeros(n, dtype=dt) for dt in dtypes)
    if not hasattr(like, "device"):
        raise ValueError("where=DEVICE without a tensor input: pass the output buffers in out=")
    import torch
    return tuple(None if dt is None else
                 torch.empty((n, dt.itemsize // 4) if dt.fields else (n,), dtype=torch.int32, device=like.device)
                 for dt in dtypes)


class BatchCalls:
    # ---- the three repeated shapes -----------------------------------------
    def _gather(self, name, rec, slots, peers, where, out, n):
        """slots + peers -> records + item_err."""
        slots, peers = _in(slots, I32, where), _in(peers, I32, where)
        n = len(slots) if n is None else n
        out = _outs(out, (rec, I32), n, where, slots)
        self._invoke(name, ptr(slots), ptr(peers), n, *map(ptr, out), where=where)
        return out

    def _per_item(self, name, rec, outs, items, where, out, n):
        """records (or slots) -> one output array per dtype of `outs`, item_err last."""
        items = _in(items, rec, where)
        n = len(items) if n is None else n
        out = _outs(out, outs, n, where, items)
        self._invoke(name, ptr(items), n, *map(ptr, out), where=where)
        return out

    def _fold(self, name, rec, items, seg_begin, where, out, n, n_seg):
        """reply records + seg_begin (NULL: one item per segment) -> flags + item_err."""
        items, sb = _in(items, rec, where), _in(seg_begin, np.int64, where)
        n = len(items) if n is None else n
        if n_seg is None:
            n_seg = 0 if sb is None else len(sb) - 1
        out = _outs(out, (I32, I32), n, where, items)
        self._invoke(name, ptr(items), n, ptr(sb), n_seg, *map(ptr, out), where=where)
        return out

    # ---- AppendEntries (raft_append_entry.go) ------------------------------
    def gather_append_args(self, slots, peers, where: int = HOST, out=None, n=None):
        return self._gather("gather_append_args", AE_ARGS, slots, peers, where, out, n)

    def process_append_replies(self, items, seg_begin=None, where: int = HOST, out=None, n=None, n_seg=None):
        return self._fold("process_append_replies", AE_RESULT, items, seg_begin, where, out, n, n_seg)

    def start(self, slots, counts=None, where: int = HOST, out=None, n=None):
        """Start (raft.go:90-104): returns (index, term, is_leader, err)."""
        slots, counts = _in(slots, I32, where), _in(counts, I32, where)
        n = len(slots) if n is None else n
        out = _outs(out, (I32,) * 4, n, where, slots)
        self._invoke("start", ptr(slots), ptr(counts), n, *map(ptr, out), where=where)
        return out

    def collect_apply(self, snapshots: bool = False, where: int = HOST, out=None):
        """Applier (raft.go:153-203): per-slot ApplyMsg index ranges [from, to];
        with snapshots=True also (snap_index, snap_term): the SnapshotValid
        message each slot sends first (snap_index -1: none)."""
        snap = I32 if snapshots else None
        out = _outs(out, (I32, I32, snap, snap), self.G * self.P, where)
        self._invoke("collect_apply", *map(ptr, out), where=where)
        return out if snapshots else out[:2]

    # ---- snapshots (raft_snapshot.go) --------------------------------------
    def snapshot(self, slots, index, where: int = HOST, out=None, n=None):
        slots, index = _in(slots, I32, where), _in(index, I32, where)
        n = len(slots) if n is None else n
        out = _outs(out, (I32,), n, where, slots)
        self._invoke("snapshot", ptr(slots), ptr(index), n, ptr(out[0]), where=where)
        return out[0]

    def gather_install_snapshot_args(self, slots, peers, where: int = HOST, out=None, n=None):
        return self._gather("gather_install_snapshot_args", IS_ARGS, slots, peers, where, out, n)

    def handle_install_snapshot(self, args, where: int = HOST, out=None, n=None):
        """HandleInstallSnapshot: (replies, flags, item_err)."""
        return self._per_item("handle_install_snapshot", IS_ARGS, (IS_REPLY, I32, I32), args, where, out, n)

    def process_install_snapshot_replies(self, items, seg_begin=None, where: int = HOST, out=None, n=None,
                                         n_seg=None):
        return self._fold("process_install_snapshot_replies", IS_RESULT, items, seg_begin, where, out, n, n_seg)

    # ---- elections (raft_election.go) --------------------------------------
    def start_election(self, slots, where: int = HOST, out=None, n=None):
        return self._per_item("start_election", I32, (RV_ARGS, I32), slots, where, out, n)

    def handle_request_vote(self, args, where: int = HOST, out=None, n=None):
        return self._per_item("handle_request_vote", RV_ARGS, (RV_REPLY, I32), args, where, out, n)

    def process_vote_replies(self, items, seg_begin=None, where: int = HOST, out=None, n=None, n_seg=None):
        return self._fold("process_vote_replies", RV_RESULT, items, seg_begin, where, out, n, n_seg)

    def export_group_status(self, leader_peer=None, where: int = HOST, out=None):
        """GetState of every group: (commit, term << 1 | is_leader)."""
        lp = _in(leader_peer, I32, where)
        out = _outs(out, (I32, I32), self.G, where, lp)
        self._invoke("export_group_status", ptr(lp), *map(ptr, out), where=where)
        return out

    # ---- persistence (raft.go:205-235) -------------------------------------
    def collect_persist(self, where: int = HOST, out=None):
        """persist_dirty of every slot (MRAFT_PERSIST_* bits), cleared on read."""
        out = _outs(out, (I32,), self.G * self.P, where)
        self._invoke("collect_persist", ptr(out[0]), where=where)
        return out[0]

    def read_persistent(self, slots):
        """SaveState (raft.go:209-216) of the given slots: (PERSISTENT records,
        packed log terms). Host arrays only."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        n = len(slots)
        hdr = np.zeros(n, dtype=PERSISTENT)
        if n == 0:
            return hdr, np.zeros(0, np.int32)
        cap = n * self.L
        terms = np.zeros(cap, np.int32)
        self._invoke("read_persistent", ptr(slots), n, ptr(hdr), ptr(terms), cap, where=None)
        used = int((hdr["last_index"].astype(np.int64) - hdr["dummy_index"] + 1).sum())
        return hdr, terms[:used].copy()

    def restore(self, hdr, terms):
        """Crash + restart (Make + readPersist, raft.go:51-87,217-235). Host arrays only."""
        hdr = np.ascontiguousarray(hdr, dtype=PERSISTENT)
        terms = np.ascontiguousarray(terms, dtype=np.int32)
        err = np.zeros(len(hdr), np.int32)
        self._invoke("restore", ptr(hdr), len(hdr), ptr(terms), len(terms), ptr(err), where=None)
        return err
