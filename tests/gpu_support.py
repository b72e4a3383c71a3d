"""Support shared by the GPU tests (imports torch lazily; not a conftest):
the device spin that proves a call only enqueues, and the child process that
runs a cases program on another build of the library."""
import contextlib
import json
import os
import subprocess
import sys


@contextlib.contextmanager
def behind_spin(engine, cycles=int(1e8), what="a call"):
    """Everything enqueued on the engine inside the block sits behind a device
    spin of `cycles` (2e8 is ~0.1 s): on exit, after the last enqueue and
    before any host wait, the stream must still be busy, so no call waited on
    the device. Then the engine is synchronised."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(engine.stream(), device=dev)
    engine.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
    yield stream
    assert not stream.query(), f"{what} waited on the device"
    engine.synchronize()


def run_cases_child(script, libpath, drop_env=()):
    """The cases program `script` in a fresh process on the library `libpath`
    (MRAFT_LIB): its last stdout line, parsed."""
    assert os.path.exists(libpath), "build() makes the test libraries"
    env = dict(os.environ, MRAFT_LIB=libpath)
    for k in drop_env:
        env.pop(k, None)
    r = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=300)
    assert r.stdout.strip(), r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0, (out, r.stderr[-3000:])
    return out
