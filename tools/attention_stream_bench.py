"""One cached decode step with the positions in device memory, beside the host-position step it stands next to (informational,
no gate).

Step times (default): the config-3 bottleneck shape -- B = 32, dim 512, H = 8, Dh = 64, depth 1, W = 128, context_x 225 -- fed
n = 1 and n = 8 new frames per call, three versions of the same step:

    (i)   host positions   ``Transformer.new_cache``, eager        (the ring write is one or two strided copies)
    (ii)  stream, eager    ``Transformer.new_stream_cache``, eager (one ``ring_write_pos`` launch, one ``stream_advance`` per call)
    (iii) stream, graph    the step of (ii) captured once (``torch.cuda.graph``) and replayed

Host clock around CALLS steps ending in a synchronise, ROUNDS rounds, the versions alternated inside every round; median / min /
max of the per-round microseconds per step.  Every version is warmed first, and all three start a round at a position beyond the
window, so every step walks the steady-state blocks.  The min..max span of a row is the spread a difference has to be read
against.

    python tools/attention_stream_bench.py > profiles/attention_stream.txt

Kernel times (``--kernels [N]``, default N = 1): the launches a kernel trace is taken of, in one process --
``attention_alibi_stream`` and ``attention_alibi_window`` at the same uniform position (tq = N, ring 225), and ``ring_write_pos``
beside the strided ``copy_`` of ``ring_write`` -- 200 calls each, alternated in blocks of 50.  Run it under a kernel-trace
profiler and read the per-kernel statistics (one N per process: the statistics are per kernel name).
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402
from audio_generation_amd.transformers import Transformer  # noqa: E402

B, DIM, H, DH, W, CTX = 32, 512, 8, 64, 128, 225
ROUNDS, CALLS = 7, 400
DEV = "cuda"


def step_times():
    torch.manual_seed(0)
    tf = Transformer(DIM, depth=1, heads=H, head_dim=DH, context_x=CTX, causal=True, window=W).to(DEV).eval()
    print(f"# host-clock times, us per step (CALLS = {CALLS} steps, then a synchronise), B={B} dim={DIM} H={H} Dh={DH} depth=1 "
          f"W={W} context_x={CTX}, fp32; {ROUNDS} rounds, versions alternated")
    print(f"# {'version':<44}{'median':>11}{'min':>11}{'max':>11}")
    for n in (1, 8):
        x = torch.randn(B, DIM, n, device=DEV)
        host, eager, graphed = tf.new_cache(B), tf.new_stream_cache(B), tf.new_stream_cache(B)
        for c in (host, eager, graphed):
            for kv in c.kv:
                kv.normal_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(3):
                tf.run_bct(x, cache=graphed)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph), torch.no_grad():
            tf.run_bct(x, cache=graphed)

        def run_host():
            tf.run_bct(x, cache=host)

        def run_eager():
            tf.run_bct(x, cache=eager)

        versions = [(f"(i)   host positions, eager        n={n}", run_host), (f"(ii)  stream cache, eager          n={n}", run_eager),
                    (f"(iii) stream cache, graph replay   n={n}", graph.replay)]
        times = {name: [] for name, _ in versions}
        with torch.no_grad():
            for name, fn in versions:
                for _ in range(50):
                    fn()
            torch.cuda.synchronize()
            for _ in range(ROUNDS):
                host.length = 1000                      # every round starts beyond the window: the steady state
                eager.pos.fill_(1000)
                graphed.pos.fill_(1000)
                for name, fn in versions:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(CALLS):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append(1e6 * (time.perf_counter() - t0) / CALLS)
        med = {}
        for name, _ in versions:
            ts = times[name]
            med[name] = statistics.median(ts)
            print(f"{name:<46}{med[name]:11.1f}{min(ts):11.1f}{max(ts):11.1f}", flush=True)
        names = [name for name, _ in versions]
        print(f"# n={n}: (ii) / (i) = {med[names[1]] / med[names[0]]:.2f}, (iii) / (i) = {med[names[2]] / med[names[0]]:.2f} (medians)")


def kernels(n):
    gen = torch.Generator().manual_seed(0)
    slopes = (2.0 ** (-8.0 / torch.arange(H, 0, -1))).to(DEV)
    attn = dict(heads=H, head_dim=DH, scale_div=DH ** 0.5)
    hd = H * DH
    ring = (0.7 * torch.randn(B, 2 * hd, CTX, generator=gen)).to(DEV)
    position = 1000
    pos = torch.full((B,), position, dtype=torch.int64, device=DEV)
    qkv = (0.7 * torch.randn(B, 3 * hd, n, generator=gen)).to(DEV)
    col0 = position % CTX
    assert col0 + n <= CTX                          # no wrap: the host-position write is one copy
    for _ in range(4):
        for _ in range(50):
            ops.attention_alibi_window(qkv, ring, slopes, **attn, window=W, q_pos0=position, ring=CTX)
        for _ in range(50):
            ops.attention_alibi_stream(qkv, ring, pos, slopes, **attn, window=W, ring=CTX)
        for _ in range(50):
            ops.ring_write(ring, qkv[:, hd:, :], col0)
        for _ in range(50):
            ops.ring_write_pos(ring, qkv[:, hd:, :], pos, CTX)
    torch.cuda.synchronize()
    print(f"kernels: done (n = {n})")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the MI355X"
    if "--kernels" in sys.argv:
        at = sys.argv.index("--kernels")
        kernels(int(sys.argv[at + 1]) if len(sys.argv) > at + 1 else 1)
    else:
        step_times()
