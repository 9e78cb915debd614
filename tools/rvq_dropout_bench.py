"""Timing of the quantiser's training-path ops with and without per-row stage counts, at the quantiser shape of
config S as bench.py builds it: the latents of its 32 clips (B = 32, D = 512, T = 225, "b c l"), its calibrated 8 x 1024 x 512
codebooks.

    python tools/rvq_dropout_bench.py [--parent-lib OTHER/libagx.so] [--calls 10] [--rounds 15]

Every figure is the median [min .. max] over ``--rounds`` timed replays, after three warm-up replays, of one captured graph of
``--calls`` back-to-back calls, in microseconds per call, all in this one process.  ``--parent-lib``: a libagx.so built from
another commit; the unstaged forward and backward are then also timed through it (the same Python wrappers, the other library
bound in their place), three times, alternated with this build's figures, to show the run-to-run spread a difference has to
be read against.  Prints the table and one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from audio_generation_amd import _lib, ops  # noqa: E402


def bind(path):
    """Another build's library under this binding: every signature it exports (a parent lacks the newest ones)."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


class Bound:
    """``with Bound(lib):`` the ops wrappers call ``lib``."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        _lib.load()
        self.saved, _lib._lib = _lib._lib, self.lib

    def __exit__(self, *exc):
        _lib._lib = self.saved


def timed(fn, calls, rounds):
    """us per call of ``fn``: (median, min, max) over ``rounds`` replays of a graph of ``calls`` calls."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            keep = fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        graph.replay()
        t1.record()
        torch.cuda.synchronize()
        us.append(1e3 * t0.elapsed_time(t1) / calls)
    del keep, graph
    return statistics.median(us), min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the MI355X: no GPU, no figure"
    dev = torch.device("cuda:0")
    model = bench.build_model(dev)
    x = bench.make_inputs(bench.BATCH_PER_GPU, 0).to(dev)
    bench.calibrate_codebooks(model, x, "latents", n_clips=8)
    quant = model.quantizer
    with torch.no_grad():
        z = model._run_encoders(x)                          # (B, D, T)
    b, d, t = z.shape
    cbs, packed, q = quant.codebooks.detach(), quant._packed_codebooks(), quant.num_quantizers
    full = torch.full((b,), q, dtype=torch.int64, device=dev)
    drop = quant.dropout_stages(b, p=1.0, generator=torch.Generator().manual_seed(0))
    g_xq, g_l = torch.randn_like(z), torch.tensor(1.0, device=dev)
    with torch.no_grad():
        _, idx, _, _ = ops.rvq_forward(z, cbs, packed, q, "b c l")
        _, idx_drop, _, _ = ops.rvq_forward(z, cbs, packed, q, "b c l", stages=drop)

    def forward(stages=None):
        return lambda: ops.rvq_forward(z, cbs, packed, q, "b c l", **({} if stages is None else {"stages": stages}))

    def backward(index, stages=None):
        return lambda: ops.rvq_backward(z, cbs, index, g_xq, g_l, "b c l", want_codebook_grad=True,
                                        **({} if stages is None else {"stages": stages}))

    parent = bind(args.parent_lib) if args.parent_lib else None
    rows, figures = [], {}

    def measure(name, fn, lib=None):
        with torch.no_grad():
            if lib is None:
                got = timed(fn, args.calls, args.rounds)
            else:
                with Bound(lib):
                    got = timed(fn, args.calls, args.rounds)
        figures.setdefault(name, []).append(got)
        rows.append(f"  {name:<58} {got[0]:9.2f} us [{got[1]:9.2f} .. {got[2]:9.2f}]")
        print(rows[-1], flush=True)

    print(f"device: {torch.cuda.get_device_name(0)}; quantiser of config S: B = {b}, T = {t}, D = {d}, K = {cbs.shape[1]}, Q = {q}, "
          f"'b c l'; dropout stages = {drop.tolist()}\nper-call time over {args.rounds} replays of a graph of {args.calls} "
          "back-to-back calls (median [min .. max])", flush=True)
    for rep in range(3):
        if parent is not None:
            measure("parent: ops.rvq_forward", forward(), parent)
            measure("parent: ops.rvq_backward", backward(idx), parent)
        if rep == 0:
            measure("this: ops.rvq_forward", forward())
            measure("this: ops.rvq_forward(stages = all Q)", forward(full))
        elif rep == 1:
            measure("this: ops.rvq_forward(stages = dropout_stages(p=1))", forward(drop))
            measure("this: ops.rvq_backward", backward(idx))
        else:
            measure("this: ops.rvq_backward(stages = all Q)", backward(idx, full))
            measure("this: ops.rvq_backward(stages = dropout_stages(p=1))", backward(idx_drop, drop))
            measure("this: ops.rvq_forward (again)", forward())
    print(json.dumps({"metric": "rvq_dropout_us_per_call", "shape": [b, t, d, int(cbs.shape[1]), q], "calls": args.calls,
                      "rounds": args.rounds, "figures": {k: [list(v) for v in vs] for k, vs in figures.items()}}), flush=True)


if __name__ == "__main__":
    main()
