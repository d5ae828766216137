"""The timing loop of the tools/*_time.py scripts, written once.  Importing it puts the repository root on sys.path.
`dev` is what supplies Event, synchronize and is_available: torch.cuda, unless a test hands in a counting stand-in."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _device(dev):
    if dev is None:
        import torch
        dev = torch.cuda
    if not dev.is_available():
        raise RuntimeError("needs a HIP device: there is no host-clock fallback")
    return dev


def event_ms(fn, batch=1, dev=None):
    """synchronise, record, `batch` calls of fn, record, synchronise: the events' time over `batch`"""
    dev = _device(dev)
    e0, e1 = dev.Event(enable_timing=True), dev.Event(enable_timing=True)
    dev.synchronize()
    e0.record()
    for _ in range(batch):
        fn()
    e1.record()
    dev.synchronize()
    return e0.elapsed_time(e1) / batch


def host_clock_ms(fn, k, warmup=0, dev=None):
    """`warmup` untimed calls, then a wall clock from an empty stream to the synchronise behind k calls: milliseconds per call"""
    dev = _device(dev)
    for _ in range(warmup):
        fn()
    dev.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    dev.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def interleaved(variants, reps, warmup):
    """variants: {name: fn} or [(name, fn)], fn() -> one sample.  Clock ramps and neighbours hit every variant of a round alike."""
    variants = list(variants.items()) if isinstance(variants, dict) else list(variants)
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    samples = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            samples[name].append(fn())
    return samples


def stat(samples):
    return {"median": statistics.median(samples), "min": min(samples), "max": max(samples)}


def emit(result, out="", indent=None):
    """`indent` is that of the printed JSON; the file is always indented"""
    print(json.dumps(result, indent=indent), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
