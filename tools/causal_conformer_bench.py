"""The streaming step of the causal Conformer conv beside the kernel it replaces on that path (informational, no gate).

The protocol of tools/conformer_bench.py: one process; every case is captured once as a graph of LAUNCHES back-to-back calls
(the Python wrapper and its allocations are in the capture, not in the replay), warmed up, and then replayed once per round
between two HIP events, the cases alternated; median [min .. max] of the per-round microseconds per call over ROUNDS rounds.
Every comparator is listed twice (``again``): the two rows were measured in the same run, alternated with everything else, and
their difference is the run-to-run spread a row has to be read against.

  (a) ``glu_dwconv_step`` at (B, C, K) and n new frames: y of the n frames and the in-place history rewrite, one launch, rows
      packed into workgroups by output
  (b) the eval-fused ``glu_dwconv`` at (B, C, T = n, K): the same arithmetic, no state, one workgroup per row.  With
      ``--parent-lib PATH`` the row is measured on that library's ``agx_glu_dwconv_forward`` (a build of the commit before the
      causal kernels), through ctypes on the same tensors; this build's own ``glu_dwconv`` is listed beside it
  (c) ``glu_dwconv_causal`` (eval fused) at the two shapes of profiles/conformer.txt beside ``glu_dwconv``: the same tile kernel
      but for ``left``
  and one cached ``ConformerBlock`` step (dim 512, n = 1) captured with ``GraphedForward``: microseconds per replay and the C
  entry calls of one step (in eval mode every entry is one launch).

    python tools/causal_conformer_bench.py [--parent-lib PATH] > profiles/causal_conformer.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import _lib, ops  # noqa: E402
from audio_generation_amd.graph import GraphedForward  # noqa: E402
from audio_generation_amd.transformers import ConformerBlock  # noqa: E402

STEP_SHAPES = [(1, 512, 17), (8, 512, 17), (32, 512, 31)]        # (B, C, K)
STEP_FRAMES = [1, 4, 16, 64]
TILE_SHAPES = [((32, 512, 1800), 10), ((32, 512, 225), 100)]     # (B, C, T), launches per graph
STEP_LAUNCHES = 100
ROUNDS = 7


def parent_forward(path):
    """``glu_dwconv(u, w, bias, bn)`` on another build of the library."""
    lib = ctypes.CDLL(path)
    fn = lib.agx_glu_dwconv_forward
    fn.restype, fn.argtypes = _lib.SIGNATURES["agx_glu_dwconv_forward"]
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(u, w, bias, bn):
        b, c2, t = u.shape
        out = torch.empty((b, c2 // 2, t), dtype=torch.float32, device=u.device)
        rc = fn(p(u), p(w), p(bias), *(p(v) for v in bn), 1e-5, p(out), b, c2 // 2, t, w.shape[-1],
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        return out
    return call


def measure(cases, launches):
    """[(name, fn)] -> {name: [microseconds per call, one per round]}."""
    graphs = []
    side = torch.cuda.Stream()
    for _, fn in cases:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(launches):
                fn()
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(ROUNDS):
        for (name, _), g in zip(cases, graphs):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            g.replay()
            stop.record()
            stop.synchronize()
            times[name].append(1e3 * start.elapsed_time(stop) / launches)
    del graphs
    return times


def show(times):
    for name, ts in times.items():
        print(f"  {name:<52}{statistics.median(ts):9.2f} us [{min(ts):9.2f} .. {max(ts):9.2f}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libagx.so of the commit before the causal kernels: comparator (b) runs on it")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    parent = parent_forward(args.parent_lib) if args.parent_lib else None
    base = "parent build" if parent else "this build"
    print(f"device: {torch.cuda.get_device_name(0)}; per-call time over {ROUNDS} replays of a graph of back-to-back launches "
          f"(median [min .. max]); comparator: glu_dwconv of {base}")
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    verdicts = []
    for b, c, k in STEP_SHAPES:
        w, bias = r(c, 1, k) / k ** 0.5, r(c)
        bn = (1.0 + 0.1 * r(c), 0.1 * r(c), 0.1 * r(c), 1.0 + 0.1 * r(c).abs())
        for n in STEP_FRAMES:
            u, hist = r(b, 2 * c, n), r(b, c, k - 1)
            same = (lambda: parent(u, w, bias, bn)) if parent else (lambda: ops.glu_dwconv(u, w, bias, bn=bn))
            cases = [(f"(b) glu_dwconv eval fused, T = n ({base})", same),
                     ("(a) glu_dwconv_step", lambda: ops.glu_dwconv_step(u, w, bias, bn, hist)),
                     (f"(b) glu_dwconv eval fused, T = n ({base}, again)", same)]
            if parent:
                cases.append(("    glu_dwconv eval fused, T = n (this build)", lambda: ops.glu_dwconv(u, w, bias, bn=bn)))
            cases.append(("    glu_dwconv_causal eval fused + hist, T = n", lambda: ops.glu_dwconv_causal(u, w, bias, bn=bn, hist=hist)))
            times = measure(cases, STEP_LAUNCHES)
            print(f"\nstep (B, C, K) = ({b}, {c}, {k}), n = {n}: {b * c * n} outputs, {STEP_LAUNCHES} launches per round")
            show(times)
            names = list(times)
            a, b1, b2 = times[names[1]], times[names[0]], times[names[2]]
            ok = statistics.median(a) <= max(max(b1), max(b2))
            verdicts.append(ok)
            print(f"  (a) / (b) = {statistics.median(a) / max(statistics.median(b1), statistics.median(b2)):.3f} .. "
                  f"{statistics.median(a) / min(statistics.median(b1), statistics.median(b2)):.3f}; (a)'s median within (b)'s [min .. max] "
                  f"or below: {'yes' if ok else 'NO'}")
    print(f"\nacceptance (a) <= (b) beyond the spread: {sum(verdicts)} of {len(verdicts)} cases")
    for (b, c, t), launches in TILE_SHAPES:
        k = 17
        u, w, bias = r(b, 2 * c, t), r(c, 1, k) / k ** 0.5, r(c)
        bn = (1.0 + 0.1 * r(c), 0.1 * r(c), 0.1 * r(c), 1.0 + 0.1 * r(c).abs())
        same = (lambda: parent(u, w, bias, bn)) if parent else (lambda: ops.glu_dwconv(u, w, bias, bn=bn))
        cases = [(f"glu_dwconv eval fused ({base})", same),
                 ("(c) glu_dwconv_causal eval fused", lambda: ops.glu_dwconv_causal(u, w, bias, bn=bn)),
                 (f"glu_dwconv eval fused ({base}, again)", same)]
        if parent:
            cases.append(("glu_dwconv eval fused (this build)", lambda: ops.glu_dwconv(u, w, bias, bn=bn)))
        times = measure(cases, launches)
        print(f"\ntile kernel (B, C, T) = ({b}, {c}, {t}), K = {k}: {launches} launches per round")
        show(times)
        names = list(times)
        cm, lo, hi = statistics.median(times[names[1]]), min(times[names[0]] + times[names[2]]), max(times[names[0]] + times[names[2]])
        print(f"  (c) median {cm:.2f} us against the comparator's [{lo:.2f} .. {hi:.2f}]: {'within or below' if cm <= hi else 'ABOVE'}")
        del u
        torch.cuda.empty_cache()
    # the whole cached block step
    for b in (1, 8):
        torch.manual_seed(0)
        block = ConformerBlock(512, kernel_size=17, context_x=256, causal=True, window=128).to(dev).eval()
        cache = block.new_stream_cache(b)
        x = r(b, 512, 1)
        calls = []
        real = _lib.check
        _lib.check = lambda rc, what: (calls.append(what), real(rc, what))[1]
        try:
            with torch.no_grad():
                block.run_bct(x, cache=cache)          # packs the weights: not counted
                calls.clear()
                block.run_bct(x, cache=cache)
        finally:
            _lib.check = real
        step = GraphedForward(lambda v: block.run_bct(v, cache=cache), x)
        ts = []
        for _ in range(ROUNDS):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(20):
                step.replay()
            stop.record()
            stop.synchronize()
            ts.append(1e3 * start.elapsed_time(stop) / 20)
        print(f"\ncached ConformerBlock step, dim 512, heads 8, K 17, window 128, n = 1, B = {b}: {len(calls)} C entry calls per step")
        print(f"  {', '.join(c.replace('agx_', '') for c in calls)}")
        print(f"  one GraphedForward replay {statistics.median(ts):9.2f} us [{min(ts):9.2f} .. {max(ts):9.2f}] (20 replays per round)")


if __name__ == "__main__":
    main()
