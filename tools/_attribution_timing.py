"""What tools/saliency_time.py, tools/path_attribution_time.py and tools/perturbation_time.py share: the fresh child process under a
time limit, the host clock around a call, the alternating rounds and the event timing of chosen entry points."""
import contextlib
import os
import statistics
import subprocess
import sys
import time


def run_in_child(script: str, limit: int, argv):
    """Run ``script --child *argv`` in a fresh process under ``timeout -k 10 <limit>`` and exit with its status."""
    rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(script), "--child"] + [str(a) for a in argv]).returncode
    if rc != 0:
        print(f"{os.path.splitext(os.path.basename(script))[0]}: ended with status {rc}", flush=True)
    sys.exit(rc)


def timed(fn) -> float:
    """Milliseconds of one call on the host clock, between two device synchronises."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(runs: dict, rounds: int, measure=timed) -> dict:
    """name -> [ms per round]: every round measures all of ``runs``, odd rounds in reverse order (A/B/.., then B/A/..)."""
    ms = {name: [] for name in runs}
    for r in range(rounds):
        for name in (tuple(runs) if r % 2 == 0 else tuple(runs)[::-1]):
            ms[name].append(measure(runs[name]))
    return ms


def summ(v) -> dict:
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


@contextlib.contextmanager
def event_timed(names, dev):
    """Inside the block every launch of the entry points ``names`` (through _lib.call) is bracketed by events on an otherwise idle
    device.  Yields the list that collects (name, arguments, microseconds)."""
    import torch
    from paths_amd import _lib
    real_call, seen = _lib.call, []

    def timed_call(name, *a):
        if name not in names:
            return real_call(name, *a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.ExternalStream(a[-1], device=dev)
        e0.record(stream)
        real_call(name, *a)
        e1.record(stream)
        torch.cuda.synchronize()
        seen.append((name, a, e0.elapsed_time(e1) * 1e3))

    _lib.call = timed_call
    try:
        yield seen
    finally:
        _lib.call = real_call
