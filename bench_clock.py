"""Secondary benchmark: the clock step (mraft_clock_step: ticker, one
election round, the sender's choice, the replication tick, the tick's timer
resets) on SURVEY.md §8d config #3 in steady state, against the sequence it
replaces when the host keeps the timers: mraft_election_rounds with one round
and an all-zero timeout mask, then mraft_replicate_tick_export with a
device-resident leader_peer. Both tick the state in place with a Start of 1-4
entries at every leader between steps, as bench.py's steady_state_config3
does (dedicated engine queue, calls enqueued back to back, an event before
and after each step's calls, the steady state = the steps after the
synthetic backlog has drained). The two sequences alternate (A B A B) on
fresh copies of the same state; the difference is the cost of the ticker and
reset launches. No oracle runs inside a timed region. Prints one JSON line.
The headline benchmark is bench.py."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--peers", type=int, default=5)
    ap.add_argument("--log", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--steady-from", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "bench_clock.py needs a GPU"
    from multiraft_amd import DEVICE, Engine, _abi, synth_seed, synth_tick_state
    lib = _abi.lib()
    G, P, L, K, ss0 = a.groups, a.peers, a.log, a.steps, a.steady_from
    dev = torch.device("cuda", 0)
    st, lp, _ = synth_tick_state(G, P, L, seed=synth_seed(3))
    master = {k: torch.from_numpy(v).to(dev) for k, v in st.items()}
    work = [{k: v.clone() for k, v in master.items()} for _ in range(2)]  # [0] clock step, [1] the sequence
    rng = np.random.default_rng(0x5EAD)
    lq = np.where(lp >= 0)[0]
    nl = len(lq)
    ldr = torch.from_numpy((lq * P + lp[lq]).astype(np.int32)).to(dev)
    cnts = [torch.from_numpy(rng.integers(1, 5, size=nl).astype(np.int32)).to(dev) for _ in range(K)]
    oi, ot, ol, oe = (torch.zeros(nl, dtype=torch.int32, device=dev) for _ in range(4))
    lp_d = torch.from_numpy(lp.astype(np.int32)).to(dev)
    zero_mask = torch.zeros((1, G), dtype=torch.uint8, device=dev)
    names = ("cand_mask", "leader_peer", "election_flags", "group_flags", "commit", "term_leader")
    out = {n: torch.zeros(G, dtype=torch.uint8 if n == "cand_mask" else torch.int32, device=dev) for n in names}
    gf, ef, commit, tl = (torch.zeros(G, dtype=torch.int32, device=dev) for _ in range(4))
    e = Engine(G, P, L, device=0, alloc=False, dedicated_queue=True)
    stream = torch.cuda.ExternalStream(e.stream(), device=dev)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def restore(c):
        for k, v in master.items():
            c[k].copy_(v)
        torch.cuda.synchronize()
        e.bind(c)

    def start(k):
        assert lib.mraft_start(e._h, ldr.data_ptr(), cnts[k].data_ptr(), nl, oi.data_ptr(), ot.data_ptr(),
                               ol.data_ptr(), oe.data_ptr(), DEVICE) == 0, _abi.last_error()

    def run(step_fn, c):
        restore(c)
        marks = [[ev(), ev()] for _ in range(K)]
        for k in range(K):
            start(k)
            marks[k][0].record(stream)
            step_fn(k)
            marks[k][1].record(stream)
        e.synchronize()
        ms = [m[0].elapsed_time(m[1]) for m in marks]
        return float(np.mean(ms[ss0:])), float(np.min(ms[ss0:])), ms

    def clock(k):
        # every Leader sends (the entries just Started go out now); timeouts far
        # beyond the run, so the election round has no candidate, as in seq()
        e.clock_step(k + 1, send_all=True, where=DEVICE, out=out)

    def seq(k):
        e.election_rounds(zero_mask, ef, where=DEVICE)
        e.replicate_tick_export(lp_d, gf, commit, tl, where=DEVICE)

    res = {"clock_step_ms": [], "sequence_ms": [], "clock_step_min_ms": [], "sequence_min_ms": []}
    # heartbeat 1, election timeouts far beyond the run (armed once: no deadline of theirs falls inside it)
    e.bind(work[0])
    e.timers_enable(1, 1, 100000, 200000, 0)
    for _ in range(a.repeats):
        m, lo, _ms = run(clock, work[0])
        res["clock_step_ms"].append(m)
        res["clock_step_min_ms"].append(lo)
        m, lo, _ms = run(seq, work[1])
        res["sequence_ms"].append(m)
        res["sequence_min_ms"].append(lo)
    # the two sequences did the same work: the same state and the same outputs
    same = all(torch.equal(work[0][k], work[1][k]) for k in master)
    # the export words are those of replica leader_peer[g]: compared where the step chose the host's leader
    agree = out["leader_peer"] == lp_d
    same_out = bool(torch.equal(out["group_flags"], gf) and torch.equal(out["commit"][agree], commit[agree]) and
                    torch.equal(out["term_leader"][agree], tl[agree]) and int(out["cand_mask"].sum()) == 0)
    n_sender, n_agree = int((out["leader_peer"] >= 0).sum()), int(agree.sum())
    mode = int(e.tick_mode())
    e.close()
    a_ms, b_ms = float(np.mean(res["clock_step_ms"])), float(np.mean(res["sequence_ms"]))
    print(json.dumps({
        "bench": "clock_step", "config": 3, "groups": G, "peers": P, "log_capacity": L, "steps": K,
        "steady_steps": K - ss0, "repeats": a.repeats, "tick_mode": mode,
        "clock_step_ms": a_ms, "parent_sequence_ms": b_ms,
        "ticker_and_reset_launches_ms": a_ms - b_ms,
        "per_repeat": res, "groups_with_sender_last_step": n_sender,
        "groups_sender_is_host_leader_last_step": n_agree,
        "same_state_as_sequence": bool(same), "same_outputs_as_sequence": same_out,
        "what": "ms per steady-state step on the device (events around the step's calls, Start excluded): "
                "clock_step_ms = one mraft_clock_step (MRAFT_DEVICE, MRAFT_CLOCK_SEND_ALL); parent_sequence_ms = "
                "mraft_election_rounds (1 round, zero mask) + mraft_replicate_tick_export"}))


if __name__ == "__main__":
    main()
