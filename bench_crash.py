"""Secondary benchmark: a crash and restart of every Leader of SURVEY.md §8d
config #3 in steady state, in place against the host round trip it replaces.
The state is the bench generator's after `--warm` clock steps (mraft_clock_step
with MRAFT_CLOCK_SEND_ALL, a Start of 1-4 entries at every leader between
steps, as bench_clock.py runs them). Two variants alternate on fresh copies of
that state, `--repeats` times:

  inplace    mraft_crash + mraft_timers_arm with MRAFT_DEVICE buffers: two
             launches enqueued on the engine stream, nothing crosses the host;
  roundtrip  mraft_read_persistent -> mraft_restore -> mraft_timers_arm with
             host buffers, the only way before mraft_crash: every Leader's log
             terms cross to the host and back, two synchronisations.

Both are timed on the host from a drained stream to a drained stream
(`wall_ms`); the in-place pair also between two events on the engine stream
(`device_ms`). After the last repeat the two results are compared: equal in
every array but log_head and log_term, which the in-place call leaves alone.
No oracle runs inside a timed region, nothing outside the tree is read.
Prints one JSON line. The headline benchmark is bench.py."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))


def measure(a):
    import torch

    assert torch.cuda.is_available(), "bench_crash.py needs a GPU"
    from multiraft_amd import DEVICE, Engine, _abi, synth_seed, synth_tick_state
    from multiraft_amd._abi import LEADER
    lib = _abi.lib()
    G, P, L = a.groups, a.peers, a.log
    dev = torch.device("cuda", 0)
    st, lp, _ = synth_tick_state(G, P, L, seed=synth_seed(3))
    work = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
    del st
    rng = np.random.default_rng(0xC4A5)
    lq = np.where(lp >= 0)[0]
    nl = len(lq)
    ldr = torch.from_numpy((lq * P + lp[lq]).astype(np.int32)).to(dev)
    oi, ot, ol, oe = (torch.zeros(nl, dtype=torch.int32, device=dev) for _ in range(4))
    e = Engine(G, P, L, device=0, alloc=False, dedicated_queue=True)
    stream = torch.cuda.ExternalStream(e.stream(), device=dev)
    e.bind(work)
    e.timers_enable(1, 1, 100000, 200000, 0)  # heartbeat 1, election timeouts far beyond the run
    for k in range(a.warm):                   # the synthetic backlog drains: steady state
        cnt = torch.from_numpy(rng.integers(1, 5, size=nl).astype(np.int32)).to(dev)
        assert lib.mraft_start(e._h, ldr.data_ptr(), cnt.data_ptr(), nl, oi.data_ptr(), ot.data_ptr(),
                               ol.data_ptr(), oe.data_ptr(), DEVICE) == 0, _abi.last_error()
        e.clock_step(k + 1, send_all=True, where=DEVICE, out={})
    e.synchronize()
    now = a.warm
    master = {k: v.clone() for k, v in work.items()}
    ed0, hd0 = e.timers_store()
    role = work["state"].cpu().numpy()
    slots = np.nonzero(role == LEADER)[0].astype(np.int32)          # every Leader
    n = len(slots)
    dslots = torch.from_numpy(slots).to(dev)
    derr = torch.zeros(n, dtype=torch.int32, device=dev)
    terms_words = int((work["last_index"].cpu().numpy()[slots].astype(np.int64) -
                       work["dummy_index"].cpu().numpy()[slots] + 1).sum())

    def fresh():
        for k, v in master.items():
            work[k].copy_(v)
        e.timers_load(ed0, hd0)
        torch.cuda.synchronize()

    def scalars():
        e.synchronize()
        return {k: v.cpu().numpy() for k, v in work.items() if k not in ("log_term", "log_head")}, e.timers_store()

    def inplace():
        fresh()
        ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
        t0 = time.perf_counter()
        ev[0].record(stream)
        e.crash(dslots, where=DEVICE, out=(derr,))
        e.timers_arm(dslots, now, where=DEVICE)
        ev[1].record(stream)
        e.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, ev[0].elapsed_time(ev[1])

    def roundtrip():
        fresh()
        t0 = time.perf_counter()
        hdr, terms = e.read_persistent(slots)
        err = e.restore(hdr, terms)
        e.timers_arm(slots, now)
        e.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert not err.any()
        return wall, None

    res = {"inplace": {"wall_ms": [], "device_ms": []}, "roundtrip": {"wall_ms": []}}
    end = {}
    for _ in range(a.repeats):
        for name, fn in (("inplace", inplace), ("roundtrip", roundtrip)):
            wall, devms = fn()
            res[name]["wall_ms"].append(wall)
            if devms is not None:
                res[name]["device_ms"].append(devms)
            end[name] = scalars()
    assert not derr.cpu().numpy().any()
    (sa, ta), (sb, tb) = end["inplace"], end["roundtrip"]
    same = all(np.array_equal(sa[k], sb[k]) for k in sa) and all(np.array_equal(x, y) for x, y in zip(ta, tb))
    e.close()
    return res, n, terms_words, bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--peers", type=int, default=5)
    ap.add_argument("--log", type=int, default=4096)
    ap.add_argument("--warm", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    res, n, words, same = measure(a)
    stat = lambda v: {"mean": float(np.mean(v)), "spread": float(np.max(v) - np.min(v)), "per_repeat": v}  # noqa: E731
    doc = {"bench": "crash_restart_every_leader", "config": 3, "groups": a.groups, "peers": a.peers,
           "log_capacity": a.log, "warm_steps": a.warm, "repeats": a.repeats, "replicas_crashed": n,
           "log_terms_of_the_crashed": words, "round_trip_mib_each_way": words * 4 / 2**20,
           "inplace_wall_ms": stat(res["inplace"]["wall_ms"]), "inplace_device_ms": stat(res["inplace"]["device_ms"]),
           "roundtrip_wall_ms": stat(res["roundtrip"]["wall_ms"]),
           "results_equal_but_for_the_ring": same,
           "what": "ms per crash + restart of every Leader: inplace = mraft_crash + mraft_timers_arm (MRAFT_DEVICE); "
                   "roundtrip = mraft_read_persistent -> mraft_restore -> mraft_timers_arm (host buffers); wall = "
                   "host clock from a drained stream to a drained stream, device = between two stream events"}
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
