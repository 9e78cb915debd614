"""The snake kernels beside kernels of the same build that move the same bytes (informational, no gate).

The protocol of profiles/conditioning.txt: one process; every case is captured once as a graph of LAUNCHES back-to-back calls
(the Python wrapper and its allocations are in the capture, not in the replay), warmed up, and then replayed once per round
between two HIP events, the cases alternated; median [min .. max] of the per-round microseconds per call over ROUNDS rounds.
Every comparator is listed twice (``again``): the two rows were measured in the same run, alternated with everything else, and
their difference is the run-to-run spread a snake row has to be read against.

Cases per shape (B, C, T), fp32, alphas near 1 and x = randn (|theta| of a few units) unless a row says otherwise:
  forward   ``film_apply`` CT without beta (reads x, writes out) against ``snake_forward``, both variants, and once with
            |theta| around 1e6, where libm's sine takes its large-argument reduction
  backward  ``sigmoid_gate_backward`` and ``film_backward`` CT (read x and dout, write dx) against ``snake_backward``: the full
            call (dx + dalpha, two launches), dx alone (frozen alphas) and dalpha alone

    python tools/snake_bench.py > profiles/snake.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402

SHAPES = [((32, 32, 72000), 20), ((32, 512, 225), 200), ((1, 32, 72000), 200)]      # (B, C, T), launches per graph
ROUNDS = 7


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    print(f"device: {torch.cuda.get_device_name(0)}; per-call time over {ROUNDS} replays of a graph of back-to-back launches "
          "(median [min .. max]),\nbytes = the tensors an op must read and write once (fp32); GB/s = bytes / median time")
    for (b, c, t), launches in SHAPES:
        gen = torch.Generator().manual_seed(0)
        x = torch.randn(b, c, t, generator=gen).to(dev)
        dout = torch.randn(b, c, t, generator=gen).to(dev)
        z = torch.randn(b, c, t, generator=gen).to(dev)
        far = (x * 4e5).contiguous()
        alpha = (1.0 + 0.1 * torch.randn(c, generator=gen)).to(dev)
        gamma, gb = torch.randn(b, c, generator=gen).to(dev), torch.randn(b, 2 * c, generator=gen).to(dev)
        n = x.numel()
        P, R = ops.SNAKE_PLAIN, ops.SNAKE_RELU
        cases = [   # (name, fn, bytes)
            ("film_apply CT, no beta", lambda: ops.film_apply(x, gamma, False, ops.FILM_CT), 8 * n),
            ("snake_forward Snek", lambda: ops.snake_forward(x, alpha, P), 8 * n),
            ("snake_forward SnekReLU", lambda: ops.snake_forward(x, alpha, R), 8 * n),
            ("snake_forward Snek, |theta| ~ 1e6", lambda: ops.snake_forward(far, alpha, P), 8 * n),
            ("film_apply CT, no beta (again)", lambda: ops.film_apply(x, gamma, False, ops.FILM_CT), 8 * n),
            ("sigmoid_gate_backward", lambda: ops.sigmoid_gate_backward(x, z, dout), 20 * n),
            ("film_backward CT", lambda: ops.film_backward(x, gb, dout, True, ops.FILM_CT), 12 * n),
            ("film_backward CT, no beta", lambda: ops.film_backward(x, gamma, dout, False, ops.FILM_CT), 12 * n),
            ("snake_backward Snek, dx + dalpha", lambda: ops.snake_backward(x, alpha, dout, P), 12 * n),
            ("snake_backward SnekReLU, dx + dalpha", lambda: ops.snake_backward(x, alpha, dout, R), 12 * n),
            ("snake_backward Snek, dx alone", lambda: ops.snake_backward(x, alpha, dout, P, want_dalpha=False), 12 * n),
            ("snake_backward Snek, dalpha alone", lambda: ops.snake_backward(x, alpha, dout, P, want_dx=False), 8 * n),
            ("snake_backward Snek, dx + dalpha, |theta| ~ 1e6", lambda: ops.snake_backward(far, alpha, dout, P), 12 * n),
            ("film_backward CT (again)", lambda: ops.film_backward(x, gb, dout, True, ops.FILM_CT), 12 * n),
            ("film_backward CT, no beta (again)", lambda: ops.film_backward(x, gamma, dout, False, ops.FILM_CT), 12 * n),
        ]
        graphs = []
        side = torch.cuda.Stream()
        for name, fn, _ in cases:
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
        times = [[] for _ in cases]
        for _ in range(ROUNDS):
            for k, g in enumerate(graphs):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                g.replay()
                stop.record()
                stop.synchronize()
                times[k].append(1e3 * start.elapsed_time(stop) / launches)
        print(f"\nshape (B, C, T) = ({b}, {c}, {t}): {n} elements, {launches} launches per round")
        med = {}
        for (name, _, nbytes), ts in zip(cases, times):
            med[name] = statistics.median(ts)
            print(f"  {name:<48}{med[name]:9.1f} us [{min(ts):9.1f} .. {max(ts):9.1f}] {nbytes / 1e6:10.1f} MB "
                  f"{nbytes / med[name] / 1e3:9.1f} GB/s", flush=True)
        fa = sorted((med["film_apply CT, no beta"], med["film_apply CT, no beta (again)"]))
        fb = sorted(med[k] for k in med if k.startswith("film_backward CT"))
        for name in ("snake_forward Snek", "snake_forward SnekReLU"):
            print(f"  {name} / film_apply CT = {med[name] / fa[1]:.3f} .. {med[name] / fa[0]:.3f}")
        for name in ("snake_backward Snek, dx + dalpha", "snake_backward SnekReLU, dx + dalpha"):
            print(f"  {name} / film_backward CT (four rows) = {med[name] / fb[-1]:.3f} .. {med[name] / fb[0]:.3f}")
        del graphs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
