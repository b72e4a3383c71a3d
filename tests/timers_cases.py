"""Seeded inputs of the timer tests (tests/test_timers_gpu.py and the CPU
coverage check in tests/test_timers_cases.py): states for mraft_ticker and
mraft_clock_step with timers loaded so that a chosen share of the slots is
due. Test infrastructure only."""
from __future__ import annotations

import numpy as np

from multiraft_amd import synth_election_state
from oracle_lib import rotate_rings
from random_states import random_tick_state
from timers_model import TimersModel

CFG = dict(seed=0xC10C, heartbeat=4, lo=6, hi=14)
NOW0 = 1000

# mraft_clock_step on arbitrary states: (P, G, send_all), three steps each
CLOCK_CASES = [(P, G, sa) for P in (1, 2, 3, 5, 8) for G in (1, 33, 300) for sa in (False, True)]
CLOCK_STEPS = 3


def clock_case_seed(P, G, send_all):
    return 31 * P + 7 * G + int(send_all)


def due_timers(rng, n, now, share):
    """Deadlines of which about `share` are due at `now`: due ones in
    {now - 2, now - 1, now} (due == now included), the others in
    {now + 1, now + 2} (due == now + 1 included)."""
    due = rng.random(n) < share
    return np.where(due, now - rng.integers(0, 3, n), now + rng.integers(1, 3, n)).astype(np.int32)


def leaders_in_place_state(G, P, L, rng, seed):
    """An election-storm state with a Leader sprinkled into 70 % of the groups
    (P = 1: half of the replicas), as mraft_ticker's tests use it."""
    from multiraft_amd._abi import LEADER
    st, _ = synth_election_state(G, P, L, seed=seed, rounds=1)
    if P > 1:
        lead = rng.random(G) < 0.7
        st["state"][np.nonzero(lead)[0] * P + rng.integers(0, P, int(lead.sum()))] = LEADER
    else:
        st["state"][rng.random(G * P) < 0.5] = LEADER
    return st


def clock_case(P, G, send_all):
    """(L, state, election_due, heartbeat_due) of one clock-step case. Even
    seeds take the tick fuzz generator's states (several Leaders per group at
    different and equal terms, followers above the leader's term, snapshot
    followers, bad-state leaders), odd seeds the election storm's; half of the
    seeds rotate the rings. A third of each timer array is due at NOW0, and the
    rest falls due over the next two steps."""
    seed = clock_case_seed(P, G, send_all)
    rng = np.random.default_rng(4400 + seed)
    L = int(rng.choice([16, 21, 32]))
    if seed % 2 == 0:
        st, _ = random_tick_state(rng, G, P, L, monotone=bool(seed % 4 == 0), snap=bool(seed % 3 == 0))
    else:
        st, _ = synth_election_state(G, P, L, seed=4400 + seed, rounds=1)
    if (seed // 2) % 2 == 0:
        st = rotate_rings(st, G, P, L, rng, frac=0.7)
    n = G * P
    ed = np.where(rng.random(n) < 1 / 3, NOW0 - rng.integers(0, 2, n), NOW0 + rng.integers(1, 4, n)).astype(np.int32)
    hd = np.where(rng.random(n) < 1 / 3, NOW0 - rng.integers(0, 2, n), NOW0 + rng.integers(1, 4, n)).astype(np.int32)
    return L, st, ed, hd


def clock_case_model(P, G, send_all):
    L, st, ed, hd = clock_case(P, G, send_all)
    m = TimersModel(G, P, L, st)
    m.enable(CFG["seed"], CFG["heartbeat"], CFG["lo"], CFG["hi"], NOW0)
    m.load(ed, hd)
    return L, st, ed, hd, m
