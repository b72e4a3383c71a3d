"""What the directed-case modules share as programs (fold_cases,
snapshot_matrix_cases, handler_cases; importable without a GPU): the loop that
runs every case on the library MRAFT_LIB names and prints one JSON line, and
the hand-built states' terms_sorted. (index_domain_cases records no ok flag
and catches nothing, so its few lines stay its own.)"""
import json
import sys

import numpy as np


def run_all(runs, run_one, on_fail_count, extra=None):
    """Every run (a tuple: the leading fields of its record) through
    run_one(*run) -> count. An AssertionError is reported on stderr and the
    run recorded as [*run, on_fail_count(*run), False], a pass as
    [*run, count, True]. Prints {"cases": [...], **extra()} as one JSON line
    and returns the exit status: 1 if any run failed."""
    out, bad = [], 0
    for run in runs:
        try:
            n, ok = run_one(*run), True
        except AssertionError as ex:
            print(f"{' '.join(map(str, run))}: {ex}", file=sys.stderr)
            n, ok, bad = on_fail_count(*run), False, bad + 1
        out.append([*run, n, ok])
    print(json.dumps({"cases": out, **(extra() if extra else {})}))
    return 1 if bad else 0


def sorted_terms(st: dict, G: int, P: int, L: int) -> np.ndarray:
    """terms_sorted as mraft_load_state computes it: the terms of Index
    dummy + 1 .. last never decrease."""
    out = np.ones(G * P, np.int32)
    for s in range(G * P):
        n = int(st["last_index"][s] - st["dummy_index"][s])
        if n >= 2:
            row = st["log_term"][s * L:(s + 1) * L]
            t = row[(int(st["log_head"][s]) + 1 + np.arange(n)) % L].astype(np.int64)
            out[s] = int((t[1:] >= t[:-1]).all())
    return out
