"""Secondary benchmark: what a reachability mask (mraft_set_reachable) costs
the steady-state clock step (mraft_clock_step with MRAFT_CLOCK_SEND_ALL) on
SURVEY.md §8d config #3, measured as bench_clock.py measures the clock step
(dedicated engine queue, calls enqueued back to back, an event before and
after each step, a Start of 1-4 entries at every leader between steps, the
steady state = the steps after the synthetic backlog has drained). Three
variants alternate on fresh copies of the same state, `--repeats` times:

  none     no mask set: the kernels as they are without the feature;
  full     a mask with every bit set: the masked kernels, every group connected;
  cut1pct  the same with one follower cut off in 1 % of the groups.

With --parent-root DIR (a built checkout of the parent commit) the variant
`none` is also measured on the parent's library, in child processes that
alternate with this tree's (one process at a time), so the no-mask figure is
compared with the parent build in the same run. No oracle runs inside a timed
region. Prints one JSON line. The headline benchmark is bench.py."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))


def measure(a, variants):
    import torch

    assert torch.cuda.is_available(), "bench_reach.py needs a GPU"
    from multiraft_amd import DEVICE, Engine, _abi, synth_seed, synth_tick_state
    lib = _abi.lib()
    G, P, L, K, ss0 = a.groups, a.peers, a.log, a.steps, a.steady_from
    dev = torch.device("cuda", 0)
    st, lp, _ = synth_tick_state(G, P, L, seed=synth_seed(3))
    master = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
    work = {k: v.clone() for k, v in master.items()}
    rng = np.random.default_rng(0x5EAD)
    lq = np.where(lp >= 0)[0]
    nl = len(lq)
    ldr = torch.from_numpy((lq * P + lp[lq]).astype(np.int32)).to(dev)
    cnts = [torch.from_numpy(rng.integers(1, 5, size=nl).astype(np.int32)).to(dev) for _ in range(K)]
    oi, ot, ol, oe = (torch.zeros(nl, dtype=torch.int32, device=dev) for _ in range(4))
    names = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")
    out = {n: torch.zeros(G, dtype=torch.uint8 if n == "cand_mask" else torch.int32, device=dev) for n in names}
    full = np.full(G, (1 << P) - 1, np.uint8)
    cut = full.copy()
    hit = lq[::100]                                        # 1 % of the groups with a leader
    cut[hit] &= ~(1 << ((lp[hit] + 1) % P)).astype(np.uint8)  # the follower after the leader
    masks = {"none": None, "full": full, "cut1pct": cut}
    e = Engine(G, P, L, device=0, alloc=False, dedicated_queue=True)
    stream = torch.cuda.ExternalStream(e.stream(), device=dev)

    def run(mask):
        for k, v in master.items():
            work[k].copy_(v)
        torch.cuda.synchronize()
        e.bind(work)
        if mask is not None or hasattr(e, "set_reachable"):
            e.set_reachable(mask)
        marks = [[torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)] for _ in range(K)]
        for k in range(K):
            assert lib.mraft_start(e._h, ldr.data_ptr(), cnts[k].data_ptr(), nl, oi.data_ptr(), ot.data_ptr(),
                                   ol.data_ptr(), oe.data_ptr(), DEVICE) == 0, _abi.last_error()
            marks[k][0].record(stream)
            e.clock_step(k + 1, send_all=True, where=DEVICE, out=out)
            marks[k][1].record(stream)
        e.synchronize()
        ms = [m[0].elapsed_time(m[1]) for m in marks]
        return float(np.mean(ms[ss0:])), int(out["commit"].to(torch.int64).sum())

    e.bind(work)
    e.timers_enable(1, 1, 100000, 200000, 0)  # heartbeat 1, election timeouts far beyond the run
    res = {v: [] for v in variants}
    commit = {}
    for _ in range(a.repeats):
        for v in variants:
            ms, c = run(masks[v])
            res[v].append(ms)
            commit[v] = c
    mode = int(e.tick_mode())
    e.close()
    return {"per_repeat_ms": res, "commit_sum_last_step": commit, "tick_mode": mode,
            "groups_cut": int(len(hit)) if "cut1pct" in variants else 0}


def child(root, a, variants):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package-root", root, "--variants", ",".join(variants),
           "--groups", str(a.groups), "--peers", str(a.peers), "--log", str(a.log), "--steps", str(a.steps),
           "--steady-from", str(a.steady_from), "--repeats", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise RuntimeError(f"bench_reach child failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--peers", type=int, default=5)
    ap.add_argument("--log", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--steady-from", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="none,full,cut1pct", help=argparse.SUPPRESS)
    a = ap.parse_args()
    variants = a.variants.split(",")
    if a.child:
        sys.path.insert(0, a.package_root)
        print(json.dumps(measure(a, variants)))
        return
    if not a.parent_root:
        sys.path.insert(0, ROOT)
        got = measure(a, variants)
        per = got["per_repeat_ms"]
        parent = None
    else:
        # this tree and the parent alternate, one process at a time
        per = {v: [] for v in variants}
        parent = []
        got = {}
        for _ in range(a.repeats):
            got = child(ROOT, a, variants)
            for v in variants:
                per[v] += got["per_repeat_ms"][v]
            parent += child(a.parent_root, a, ["none"])["per_repeat_ms"]["none"]
    mean = {v: float(np.mean(per[v])) for v in variants}
    spread = {v: float(np.max(per[v]) - np.min(per[v])) for v in variants}
    doc = {"bench": "reach_clock_step", "config": 3, "groups": a.groups, "peers": a.peers, "log_capacity": a.log,
           "steps": a.steps, "steady_steps": a.steps - a.steady_from, "repeats": a.repeats,
           "tick_mode": got.get("tick_mode"), "groups_cut": got.get("groups_cut"),
           "ms": mean, "repeat_spread_ms": spread, "per_repeat_ms": per,
           "full_mask_over_none_ms": mean.get("full", 0.0) - mean.get("none", 0.0),
           "cut1pct_over_none_ms": mean.get("cut1pct", 0.0) - mean.get("none", 0.0),
           "commit_sum_last_step": got.get("commit_sum_last_step"),
           "what": "ms per steady-state mraft_clock_step (MRAFT_DEVICE, MRAFT_CLOCK_SEND_ALL; events around the "
                   "step, Start excluded): none = no mask set, full = all-ones mask set, cut1pct = one follower "
                   "cut off in 1 % of the groups"}
    if parent is not None:
        doc["parent_none_ms"] = float(np.mean(parent))
        doc["parent_none_per_repeat_ms"] = parent
        doc["parent_none_spread_ms"] = float(np.max(parent) - np.min(parent))
        doc["none_minus_parent_ms"] = mean["none"] - doc["parent_none_ms"]
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
