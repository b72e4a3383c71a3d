"""ctypes wrapper of the CPU oracle (oracle/liboracle.so) with the same method
names as multiraft_amd.engine.Engine. Test infrastructure only."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from multiraft_amd._abi import AE_ARGS, AE_REPLY, AE_RESULT, HOST, MraftSoa, ptr, soa_of
from multiraft_amd._calls import BatchCalls
from multiraft_amd.engine import copy_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PATH = os.path.join(ROOT, "oracle", "liboracle.so")


class OraEngine(ctypes.Structure):
    _fields_ = [("G", ctypes.c_int32), ("P", ctypes.c_int32), ("L", ctypes.c_int32),
                ("s", MraftSoa)]


_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
_E = ctypes.POINTER(OraEngine)
# argument types of every symbol used; the ora_<name> of a BatchCalls method has
# mraft_<name>'s without the trailing `where` (tests/test_calls.py)
SIGS = {
    "ora_count_enable": [_E], "ora_count_disable": [], "ora_count_result": [_vp],
    "ora_count_result_lines": [_i32, _vp],
    "ora_compute_terms_sorted": [_E],
    "ora_gather_append_args": [_E, _vp, _vp, _i64, _vp, _vp],
    "ora_handle_append_entries": [_E, _vp, _i64, _vp, _i64, _vp, _vp],
    "ora_process_append_replies": [_E, _vp, _i64, _vp, _i64, _vp, _vp],
    "ora_replicate_tick": [_E, _vp, _vp],
    "ora_replicate_tick_mt": [_E, _vp, _vp, _i32],
    "ora_start": [_E, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "ora_collect_apply": [_E, _vp, _vp, _vp, _vp],
    "ora_start_election": [_E, _vp, _i64, _vp, _vp],
    "ora_handle_request_vote": [_E, _vp, _i64, _vp, _vp],
    "ora_process_vote_replies": [_E, _vp, _i64, _vp, _i64, _vp, _vp],
    "ora_export_group_status": [_E, _vp, _vp, _vp],
    "ora_election_rounds": [_E, _vp, _i32, _vp],
    "ora_election_rounds_mt": [_E, _vp, _i32, _vp, _i32],
    "ora_snapshot": [_E, _vp, _vp, _i64, _vp],
    "ora_gather_install_snapshot_args": [_E, _vp, _vp, _i64, _vp, _vp],
    "ora_handle_install_snapshot": [_E, _vp, _i64, _vp, _vp, _vp],
    "ora_process_install_snapshot_replies": [_E, _vp, _i64, _vp, _i64, _vp, _vp],
    "ora_collect_persist": [_E, _vp],
    "ora_read_persistent": [_E, _vp, _i64, _vp, _vp, _i64],
    "ora_restore": [_E, _vp, _i64, _vp, _i64, _vp],
    "goshape_build": [_i32, _i32, _i32, ctypes.POINTER(MraftSoa)],
    "goshape_store": [_vp, ctypes.POINTER(MraftSoa)],
    "goshape_free": [_vp],
    "goshape_tick": [_vp, _vp, _i32],
    "goshape_reset": [_vp, ctypes.POINTER(MraftSoa), _i32],
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = ctypes.CDLL(_PATH)
        for n, a in SIGS.items():
            f = getattr(l, n)
            f.argtypes = a
            f.restype = None if n in ("ora_count_disable", "ora_count_result", "ora_count_result_lines", "goshape_store",
                                      "goshape_free", "goshape_reset", "ora_compute_terms_sorted") else ctypes.c_int
        l.goshape_build.restype = ctypes.c_void_p
        l.goshape_tick.restype = ctypes.c_int64
        _lib = l
    return _lib


class Oracle(BatchCalls):
    """CPU restatement with the Engine's interface (the batched message-path
    calls are BatchCalls', host arrays only); operates on its own copy of the
    state."""

    def __init__(self, G: int, P: int, L: int, st: dict):
        self.G, self.P, self.L = G, P, L
        self.st = copy_state(st)
        self.st.setdefault("log_head", np.zeros(G * P, np.int32))  # fixtures made before the ring
        self.st.setdefault("has_snapshot", np.zeros(G * P, np.int32))
        self.st["terms_sorted"] = np.zeros(G * P, np.int32)
        self._e = OraEngine(G, P, L, soa_of(self.st))
        lib().ora_compute_terms_sorted(ctypes.byref(self._e))  # as mraft_load_state does

    def _invoke(self, name, *c_args, where=HOST):
        if where not in (None, HOST):
            raise ValueError(f"ora_{name}: the oracle takes host arrays only")
        rc = getattr(lib(), "ora_" + name)(ctypes.byref(self._e), *c_args)
        assert rc == 0, f"ora_{name} failed ({rc})"

    def state(self) -> dict:
        return self.st

    def load_state(self, st: dict):
        """Replace the whole state in place, as mraft_load_state does
        (terms_sorted recomputed from the logs)."""
        for k, v in self.st.items():
            if k != "terms_sorted":
                v[:] = st[k]
        lib().ora_compute_terms_sorted(ctypes.byref(self._e))

    def replicate_tick(self, leader_peer, nthreads: int = 1):
        lp = np.ascontiguousarray(leader_peer, dtype=np.int32)
        gf = np.zeros(self.G, dtype=np.int32)
        if nthreads > 1:
            lib().ora_replicate_tick_mt(ctypes.byref(self._e), ptr(lp), ptr(gf), nthreads)
        else:
            lib().ora_replicate_tick(ctypes.byref(self._e), ptr(lp), ptr(gf))
        return gf

    def replicate_tick_count(self, leader_peer, line_words=()):
        """Counts on a scratch copy (the state is left untouched). With
        line_words, also {line_words: (read lines, written lines)}."""
        scratch = Oracle(self.G, self.P, self.L, self.st)
        L = lib()
        L.ora_count_enable(ctypes.byref(scratch._e))
        lines = {}
        try:
            gf = scratch.replicate_tick(leader_peer)
            out = (ctypes.c_int64 * 2)()
            L.ora_count_result(out)
            for lw in line_words:
                o2 = (ctypes.c_int64 * 2)()
                L.ora_count_result_lines(lw, o2)
                lines[lw] = (int(o2[0]), int(o2[1]))
        finally:
            L.ora_count_disable()
        active = int(np.count_nonzero(gf & 1))
        if line_words:
            return int(out[0]), int(out[1]), active, lines
        return int(out[0]), int(out[1]), active

    def handle_append_entries(self, args, entry_terms):
        args = np.ascontiguousarray(args, dtype=AE_ARGS)
        n = len(args)
        rep = np.zeros(n, dtype=AE_REPLY)
        err = np.zeros(n, dtype=np.int32)
        et = None if entry_terms is None else np.ascontiguousarray(entry_terms, dtype=np.int32)
        self._invoke("handle_append_entries", ptr(args), n, ptr(et), 0 if et is None else len(et), ptr(rep), ptr(err))
        return rep, err

    def store_state(self):
        return copy_state(self.st)

    def scalar_state(self):
        """The live state arrays (read-only use: the harness's mirror)."""
        return self.st

    def election_rounds(self, cand_mask, nthreads: int = 1):
        m = np.ascontiguousarray(cand_mask, dtype=np.uint8)
        gf = np.zeros(self.G, np.int32)
        lib().ora_election_rounds_mt(ctypes.byref(self._e), ptr(m), m.shape[0], ptr(gf), nthreads)
        return gf


def logical_logs(st: dict, G: int, P: int, L: int):
    """[G*P, L] view of every replica's log in Index order: row r, column k =
    the term of Index dummy + k (the ring of include/mraft.h unrolled from
    log_head); columns past last - dummy are dead slots."""
    lt = st["log_term"].reshape(G * P, L)
    h = st["log_head"] if "log_head" in st else np.zeros(G * P, np.int32)
    cols = (h[:, None].astype(np.int64) + np.arange(L)[None, :]) % L
    return np.take_along_axis(lt, cols, axis=1)


def assert_states_equal(a: dict, b: dict, G: int, P: int, L: int, ctx: str = "", heads: bool = True):
    """Compare two state images. Logs are compared in Index order over the
    live entries [dummy, last] of every replica (slots past lastIndex are dead:
    the reference's slice has no such slots). heads=False skips the ring
    positions themselves (the Python restatement has no ring)."""
    for st in (a, b):
        assert_terms_sorted_sound(st, G, P, L, ctx)
    for k in a:
        if k == "log_term" or (k == "log_head" and not heads) or k not in b:
            continue
        if not np.array_equal(a[k], b[k]):
            bad = np.nonzero(a[k] != b[k])[0][:8]
            raise AssertionError(f"{ctx}: {k} differs at {bad}: {a[k][bad]} vs {b[k][bad]}")
    la = logical_logs(a, G, P, L)
    lb = logical_logs(b, G, P, L)
    live = a["last_index"] - a["dummy_index"]
    mask = np.arange(L)[None, :] <= live[:, None]
    if not np.array_equal(np.where(mask, la, 0), np.where(mask, lb, 0)):
        rows = np.nonzero((np.where(mask, la, 0) != np.where(mask, lb, 0)).any(axis=1))[0][:8]
        raise AssertionError(f"{ctx}: log_term differs in replicas {rows}")


def terms_sorted_exact(st: dict, G: int, P: int, L: int) -> np.ndarray:
    """Whether each replica's terms of Index dummy+1 .. last never decrease."""
    logs = logical_logs(st, G, P, L).astype(np.int64)
    live = (st["last_index"] - st["dummy_index"]).astype(np.int64)  # entries after the dummy
    k = np.arange(1, L)[None, :]
    desc = (logs[:, 1:-1] > logs[:, 2:]) if L > 2 else np.zeros((G * P, 0), bool)
    desc = desc & (k[:, :-1] < live[:, None]) if L > 2 else desc
    return (~desc.any(axis=1)).astype(np.int32)


def assert_terms_sorted_sound(st: dict, G: int, P: int, L: int, ctx: str = ""):
    """terms_sorted is a proof (include/mraft.h): 1 only where the terms after
    the dummy really never decrease."""
    if "terms_sorted" not in st:
        return
    bad = np.nonzero((st["terms_sorted"] != 0) & (terms_sorted_exact(st, G, P, L) == 0))[0]
    if len(bad):
        raise AssertionError(f"{ctx}: terms_sorted claims sorted terms in replicas {bad[:8]}")


def rotate_rings(st: dict, G: int, P: int, L: int, rng, frac: float = 1.0) -> dict:
    """The same logical state with every replica's ring started at a random
    head (a fraction `frac` of the replicas): row contents rotated so Index
    dummy + k sits at (head + k) mod L. Exercises the wrap in every kernel."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    logs = logical_logs(st, G, P, L)
    h = rng.integers(0, L, G * P).astype(np.int32)
    h[rng.random(G * P) >= frac] = 0
    cols = (h[:, None].astype(np.int64) + np.arange(L)[None, :]) % L
    lt = np.empty_like(logs)
    np.put_along_axis(lt, cols, logs, axis=1)
    out["log_term"] = lt.reshape(-1)
    out["log_head"] = h
    return out


class GoShaped:
    """The tick on the reference's own data shapes (oracle/mraft_goshape.c):
    the CPU baseline's Go-shaped variant. Built from a SoA image (untimed)."""

    def __init__(self, G: int, P: int, L: int, st: dict):
        self.G, self.P, self.L = G, P, L
        self._st = st
        self._soa = soa_of(st)
        self._c = lib().goshape_build(G, P, L, ctypes.byref(self._soa))

    def replicate_tick(self, leader_peer, nthreads: int = 1) -> int:
        lp = np.ascontiguousarray(leader_peer, dtype=np.int32)
        return int(lib().goshape_tick(self._c, ptr(lp), nthreads))

    def reset(self, nthreads: int = 1):
        """Back to the state it was built from (slices keep their capacity)."""
        lib().goshape_reset(self._c, ctypes.byref(self._soa), nthreads)

    def state(self) -> dict:
        out = copy_state(self._st)
        soa = soa_of(out)
        lib().goshape_store(self._c, ctypes.byref(soa))
        return out

    def close(self):
        if self._c:
            lib().goshape_free(self._c)
            self._c = None

    def __del__(self):
        self.close()


def random_reply_segments(st: dict, G: int, P: int, lp: np.ndarray, seed: int, max_len: int = 150):
    """Reply batches for process_append_replies beyond what a3 produces: per
    leader slot a segment of 0..max_len replies in arrival order (repeats of a
    peer, stale and higher terms, failures, successes whose matchIndex moves
    up and down), so a1 runs many times per segment, over logs whose tail may
    not carry the current term (the Figure-8 scan). Returns items, seg_begin."""
    rng = np.random.default_rng(seed)
    L = st["log_term"].size // (G * P)
    out = []
    seg = [0]
    for g in range(G):
        if lp[g] < 0 or P < 2:
            continue
        s = g * P + int(lp[g])
        k = int(rng.integers(0, max_len + 1)) if rng.random() < 0.9 else 0
        T, last = int(st["current_term"][s]), int(st["last_index"][s])
        nxt = st["next_index"][s * P:(s + 1) * P].astype(np.int64).copy()
        for _ in range(k):
            p = int(rng.integers(0, P - 1))
            p = p if p < s % P else p + 1
            r = np.zeros(1, dtype=AE_RESULT)[0]
            r["slot"], r["peer"] = s, p
            u = rng.random()
            r["args_term"] = T if u < 0.9 else T - 1
            prev = int(nxt[p]) - 1 if rng.random() < 0.8 else int(rng.integers(0, last + 1))
            r["args_prev_log_index"] = prev
            n = int(rng.integers(0, max(1, last - prev + 1))) if prev <= last else 0
            r["args_n_entries"] = n
            v = rng.random()
            r["reply_term"] = T if v < 0.995 else (T + 1 if v < 0.997 else T - 1)
            ok = rng.random() < 0.7
            r["reply_success"] = int(ok)
            r["reply_conflict_index"] = int(rng.integers(1, max(2, prev + 2)))
            if ok and prev == nxt[p] - 1:
                nxt[p] = prev + n + 1
            elif prev == nxt[p] - 1:
                nxt[p] = r["reply_conflict_index"]
            out.append(r)
        seg.append(len(out))
    items = np.array(out, dtype=AE_RESULT) if out else np.zeros(0, dtype=AE_RESULT)
    return items, np.array(seg, dtype=np.int64)
