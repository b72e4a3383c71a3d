"""bench.py's output dump (--dump-outputs) and the split between a plain run
and --full: the dump is float64, whole for small arrays and a fixed seeded
sample for large ones; a plain run carries the headline fields and none of the
--full legs; and on a GPU the dumped last step equals the oracle's tick of the
same seeded workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import Oracle, assert_states_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_whole_and_sampled(tmp_path):
    import torch

    import bench
    n_big = bench.DUMP_MAX_ELEMS + 12345
    rng = np.random.default_rng(7)
    small = rng.integers(-2**31, 2**31, 1000).astype(np.int32)
    big = rng.integers(-2**31, 2**31, n_big).astype(np.int32)
    arrays = {"small": torch.from_numpy(small), "big": torch.from_numpy(big)}
    total = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float64 and b.dtype == np.float64
    assert total == s.nbytes + b.nbytes
    assert np.array_equal(s, small.astype(np.float64))  # int32 is exact in float64
    assert b.shape == (bench.DUMP_MAX_ELEMS,)
    # the sample: the same sorted indices in every run, from the seed and the name alone
    idx = np.sort(np.random.default_rng([bench.DUMP_SEED, *b"big"]).integers(0, n_big, bench.DUMP_MAX_ELEMS))
    assert np.array_equal(b, big[idx].astype(np.float64))
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    # config #3's 18 arrays at the cap stay under the 64 MB limit
    assert 18 * bench.DUMP_MAX_ELEMS * 8 <= 64 * 10**6


def test_dry_run_accepts_full_and_dump_outputs(tmp_path):
    out = _bench("--dry-run", "--log", "64", "--full", "--dump-outputs", str(tmp_path / "d"))
    assert out["dry_run"] and out["value"] is None and out["steps"] == 20
    assert not (tmp_path / "d").exists()  # no GPU step ran: nothing to write


@pytest.mark.gpu
def test_plain_run_is_lean_and_dump_equals_oracle_gpu(tmp_path):
    """A plain run on a small workload (256 x 5 x 256: every array under the
    sample cap, two tick shards, so the dump is the whole last step): the
    headline fields, none of the --full legs, --steps timed steps; the dumped
    flags, export words and state equal the oracle's tick of the same seeded
    state."""
    from multiraft_amd import synth_seed, synth_tick_state
    G, P, L, K = 256, 5, 256, 3
    d = tmp_path / "out"
    out = _bench("--gpus", "1", "--steps", str(K), "--warmup", "1", "--groups", str(G), "--log", str(L),
                 "--dump-outputs", str(d))
    assert out["steps"] == K and out["warmup"] == 1 and out["unit"] == "decisions/s"
    assert out["higher_is_better"] is True and out["dtype"] == "int32"
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(G / (out["ms_per_step"] / 1e3))
    assert len(out["roofline"]["kernel_ms_steps_apportioned"]) == K
    assert out["cpu_baseline"] is None and "secondary" not in out
    assert "placement_probe" not in out["roofline"]

    st, lp, _ = synth_tick_state(G, P, L, seed=synth_seed(3))
    ora = Oracle(G, P, L, st)
    flags = ora.replicate_tick(lp)
    commit, term_leader = ora.export_group_status(lp)
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 * 10**6
    assert np.array_equal(got["group_flags"], flags)
    assert np.array_equal(got["status_commit"], commit)
    assert np.array_equal(got["status_term_leader"], term_leader)
    state = {k[len("state_"):]: v.astype(np.int32) for k, v in got.items() if k.startswith("state_")}
    assert set(state) == set(st)
    assert_states_equal(state, ora.state(), G, P, L, "bench dump")
