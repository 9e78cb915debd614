"""Attention with dropout beside its cross-attention twin, and the elementwise dropout kernel (informational, no gate).

The protocol of profiles/cross_attention.txt: one process, HIP events, 20 warm-up calls per case, then ROUNDS rounds; in every
round each case is timed over CALLS back-to-back calls between two events, the cases alternated; median / min / max of the
per-round microseconds per call (the Python wrapper, which allocates outputs and workspace per call, included).

    python tools/attention_dropout_bench.py > profiles/attention_dropout.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import ops  # noqa: E402

B, H, DH, TQ, TK, P = 32, 8, 64, 225, 225, 0.1
ELEMENTWISE = (32, 512, 225)
WARMUP, ROUNDS, CALLS = 20, 5, 200
SEED = 0x243F6A8885A308D3


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    q = (0.7 * torch.randn(B, H * DH, TQ, generator=gen)).to(dev)
    kv = (0.7 * torch.randn(B, 2 * H * DH, TK, generator=gen)).to(dev)
    dout = torch.randn(B, H * DH, TQ, generator=gen).to(dev)
    slopes = (2.0 ** (-8.0 / torch.arange(H, 0, -1))).to(dev)
    attn = dict(heads=H, head_dim=DH, scale_div=DH ** 0.5)
    drop = dict(p=P, seed=SEED, stream_id=0)
    out_c = ops.attention_alibi_cross(q, kv, slopes, **attn)
    out_d = ops.attention_alibi_dropout(q, kv, slopes, **attn, **drop)
    x, res = torch.randn(ELEMENTWISE, generator=gen).to(dev), torch.randn(ELEMENTWISE, generator=gen).to(dev)
    buf = torch.empty_like(x)
    n = x.numel()
    cases = [
        (f"cross fwd ({TQ},{TK})", lambda: ops.attention_alibi_cross(q, kv, slopes, **attn), None),
        (f"dropout fwd ({TQ},{TK}) p={P}", lambda: ops.attention_alibi_dropout(q, kv, slopes, **attn, **drop), None),
        (f"dropout fwd ({TQ},{TK}) p=0", lambda: ops.attention_alibi_dropout(q, kv, slopes, **attn, p=0.0, seed=SEED, stream_id=0), None),
        (f"cross bwd ({TQ},{TK})", lambda: ops.attention_alibi_cross_backward(q, kv, slopes, out_c, dout, **attn), None),
        (f"dropout bwd ({TQ},{TK}) p={P}", lambda: ops.attention_alibi_dropout_backward(q, kv, slopes, out_d, dout, **attn, **drop), None),
        (f"dropout_add + res {ELEMENTWISE}", lambda: ops.dropout_add(x, res, P, SEED, 1, out=buf), 12 * n),
        (f"dropout_add in place {ELEMENTWISE}", lambda: ops.dropout_add(buf, None, P, SEED, 2, out=buf), 8 * n),
    ]
    for _, fn, _ in cases:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):
        for name, fn, _ in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(CALLS):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(1e3 * start.elapsed_time(stop) / CALLS)
    print(f"# HIP-event times, us per call (wrapper included), B={B} H={H} Dh={DH}, fp32; {ROUNDS} rounds x {CALLS} calls, cases alternated")
    print(f"# {'case':<44}{'median':>10}{'min':>10}{'max':>10}{'GB/s':>10}")
    for name, _, nbytes in cases:
        t = times[name]
        med = statistics.median(t)
        rate = f"{nbytes / med / 1e3:10.0f}" if nbytes else ""
        print(f"{name:<46}{med:10.1f}{min(t):10.1f}{max(t):10.1f}{rate}")


if __name__ == "__main__":
    main()
