"""Host time of one ``ops.attention_alibi_stream(counts=)`` call, the wrapper the cached decode step runs once per layer and step,
for several versions of ``ops.py`` side by side (no GPU, no kernel: informational, no gate).

    python tools/attention_wrapper_cost.py parent_a OLD/ops.py parent_b OLD/ops.py new audio_generation_amd/ops.py

Every file is loaded as a module of its own inside the package; ``_lib.load`` answers a library whose every symbol returns 0,
``_need_gpu`` and ``_stream`` are replaced as ``tests/test_attention_calls_cpu.py`` replaces them, no observer is set.  The
operands are the shapes of that test (B = 2, H = 2, Dh = 16, Tq = 5, a 96-channel qkv tensor as ``q``, cap = 20).  ``timeit`` of
CALLS calls, REPEATS times per version with the versions alternated inside every repeat, so that a drift of the machine meets
them alike; median (min, max) of the per-repeat microseconds per call.  Name one file twice: the gap between its two medians is
the spread a difference has to be read against.
"""
import ctypes
import importlib.util
import os
import statistics
import sys
import timeit

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import _lib  # noqa: E402

CALLS, REPEATS = 20000, 41


class NoLibrary:
    def __getattr__(self, symbol):
        setattr(self, symbol, lambda *args: 0)
        return getattr(self, symbol)


def stream_call(index, path):
    spec = importlib.util.spec_from_file_location(f"audio_generation_amd._ops_timed_{index}", path)
    ops = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ops)
    null = ctypes.c_void_p(0)
    ops._need_gpu = lambda *tensors: None
    ops._stream = lambda: null
    q, kv, slopes = torch.zeros(2, 96, 5), torch.zeros(2, 64, 20), torch.ones(2)
    pos, counts = torch.tensor([3, 4]), torch.tensor([5, 0])
    return lambda: ops.attention_alibi_stream(q, kv, pos, slopes, 2, 16, 4.0, 4, 16, counts=counts)


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        raise SystemExit(__doc__)
    library = NoLibrary()
    _lib.load = lambda: library
    labels, calls = argv[0::2], [stream_call(i, path) for i, path in enumerate(argv[1::2])]
    for call in calls:
        call()
    times = [[] for _ in calls]
    for _ in range(REPEATS):
        for row, call in zip(times, calls):
            row.append(1e6 * timeit.timeit(call, number=CALLS) / CALLS)
    for label, row in zip(labels, times):
        print(f"{label}: median {statistics.median(row):.3f} us per call (min {min(row):.3f}, max {max(row):.3f}; {REPEATS} x {CALLS} calls)")


if __name__ == "__main__":
    main(sys.argv[1:])
