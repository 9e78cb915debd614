"""The generation step of a ``CodePrior`` (informational, no gate).

Step times (default): B = 32, Q = 8, K = 1024, dim = 512, depth = 4, heads = 8 of 64, window = 256, context_x = 512.  One
``CodePrior.step`` -- snapshot, embedding of the carried codes, four cached Transformer layers, LayerNorm, head, sampler --
eager and captured once (``GraphedForward``) and replayed.  Host clock around CALLS steps ending in a synchronise, ROUNDS rounds,
the two versions alternated inside every round; median / min / max of the per-round microseconds per step, and frames per second
(B frames per step).  Every round starts beyond the window, so every step walks the steady-state blocks.

    python tools/prior_bench.py > profiles/prior.txt

Kernel times (``--kernels``): the new kernels alone, 200 calls each at the shapes of that step and of a training batch
(B = 32, T = 225) -- ``codes_embed`` (n = 1 and n = 225), ``codes_sample`` (n = 1), ``codes_cross_entropy`` and its backward,
``codes_embed_backward``.  Run it under a kernel-trace profiler (``rocprofv3 --kernel-trace --stats -- python tools/prior_bench.py
--kernels``) and read the per-kernel statistics; the run prints the bytes each kernel must move, to set the times against.
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402
from audio_generation_amd.graph import GraphedForward  # noqa: E402
from audio_generation_amd.prior import CodePrior  # noqa: E402

B, Q, K, DIM, DEPTH, H, DH, W, CTX, T = 32, 8, 1024, 512, 4, 8, 64, 256, 512, 225
ROUNDS, CALLS = 7, 200
DEV = "cuda"


def step_times():
    torch.manual_seed(0)
    model = CodePrior(Q, K, DIM, DEPTH, H, DH, W, CTX).to(DEV).eval()
    ones = torch.ones(B, dtype=torch.int64, device=DEV)
    eager, graphed = model.new_state(B, seed=1), model.new_state(B, seed=1)
    for st in (eager, graphed):
        st.set_sampling(temperature=0.9, top_k=250, top_p=0.95)
        for kv in st.cache.kv:
            kv.normal_()
    graph = GraphedForward(lambda c: model.step(graphed, counts=c), ones)
    versions = [("step, eager", lambda: model.step(eager, counts=ones)), ("step, graph replay", graph.replay)]
    print(f"# host-clock times, us per step (CALLS = {CALLS} steps, then a synchronise), B={B} Q={Q} K={K} dim={DIM} depth={DEPTH} "
          f"H={H} Dh={DH} W={W} context_x={CTX}, fp32, temperature 0.9 top_k 250 top_p 0.95; {ROUNDS} rounds, versions alternated")
    print(f"# {'version':<28}{'median':>11}{'min':>11}{'max':>11}{'ms/step':>11}{'frames/s':>13}")
    times = {name: [] for name, _ in versions}
    for name, fn in versions:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for st in (eager, graphed):
            st.cache.pos.fill_(1000)                    # beyond the window: the steady state
        for name, fn in versions:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0) / CALLS)
    for name, _ in versions:
        ts = times[name]
        med = statistics.median(ts)
        print(f"{name:<30}{med:11.1f}{min(ts):11.1f}{max(ts):11.1f}{med / 1e3:11.3f}{B * 1e6 / med:13.0f}", flush=True)
    launches = 3 + 8 * DEPTH + 5
    print(f"# a step is {launches} launches (copy, embed, mask, {DEPTH} x 8 layer launches, advance, mask, LayerNorm, head, sampler): "
          "compare the replayed step with launches x the per-launch floor before reading it as kernel time")


def kernels():
    gen = torch.Generator().manual_seed(0)
    tables = torch.randn(Q, K + 1, DIM, generator=gen).to(DEV)
    sizes = (K,) * Q
    rows = []
    for n in (1, T):
        index = torch.randint(0, K, (B, n, Q), generator=gen).to(DEV)
        for _ in range(200):
            out = ops.codes_embed(index, tables)
        rows.append((f"codes_embed n={n}", 4 * B * n * Q * DIM + 8 * B * n * Q + 4 * out.numel()))
    logits1 = (3.0 * torch.randn(B, Q * K, 1, generator=gen)).to(DEV)
    i64 = torch.arange(B, dtype=torch.int64, device=DEV)
    tau, tp = torch.full((B,), 0.9, device=DEV), torch.full((B,), 0.95, device=DEV)
    tk = torch.full((B,), 250, dtype=torch.int64, device=DEV)
    for _ in range(200):
        ops.codes_sample(logits1, Q, i64, i64, tau, tk, tp, sizes)
    rows.append(("codes_sample n=1", 4 * logits1.numel() + 8 * B * Q))
    logits = torch.randn(B, Q * K, T, generator=gen).to(DEV)
    target = torch.randint(0, K, (B, T, Q), generator=gen).to(DEV)
    g = torch.ones((), device=DEV)
    for _ in range(200):
        loss, nll, lse, n_live = ops.codes_cross_entropy(logits, target, sizes)
    rows.append((f"codes_cross_entropy T={T}", 4 * logits.numel() + 16 * target.numel()))
    for _ in range(200):
        ops.codes_cross_entropy_backward(logits, target, lse, n_live, g, sizes)
    rows.append((f"codes_cross_entropy_backward T={T}", 8 * logits.numel() + 12 * target.numel()))
    dout = torch.randn(B, DIM, T, generator=gen).to(DEV)
    for _ in range(200):
        ops.codes_embed_backward(dout, target, K + 1)
    f = B * T
    rows.append((f"codes_embed_backward T={T} (three kernels)", 8 * f * DIM + 12 * f * Q + 4 * f * Q * DIM + 4 * Q * (K + 1) * DIM))
    torch.cuda.synchronize()
    print("# bytes each op must move (reads + writes, every operand once); 200 calls each")
    for name, nbytes in rows:
        print(f"{name:<48}{nbytes:>14d} bytes")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the MI355X"
    if "--kernels" in sys.argv:
        kernels()
    else:
        step_times()
