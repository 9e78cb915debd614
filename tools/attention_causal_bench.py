"""Causal attention beside the symmetric self-attention kernels it replaces (informational, no gate).

The protocol of profiles/attention_dropout.txt: one process, HIP events, warm-up calls per case, then ROUNDS rounds; in every
round each case is timed over its CALLS back-to-back calls between two events, the cases alternated; median / min / max of the
per-round microseconds per call (the Python wrapper, which allocates outputs and workspace per call, included).  Every
baseline is listed twice (``again``): the two rows were measured in the same run, alternated with everything else, and their
difference is the run-to-run spread a causal row has to be read against.

Cases per T: the symmetric online-softmax forward ``attention_alibi(flash=True)`` and ``attention_alibi_causal``; the symmetric
split backward (``agx_attention_alibi_backward_ex``, called as ``ops.attention_alibi_backward`` calls it where it has no
single-launch kernel) and ``attention_alibi_causal_backward``; at the longest T one cached step, tq = 1 on tk = T keys.

    python tools/attention_causal_bench.py > profiles/attention_causal.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audio_generation_amd import _lib, ops  # noqa: E402

B, H, DH = 32, 8, 64
LENGTHS = (225, 1125)
ROUNDS = 5


def split_backward(qkv, slopes, out, dout):
    """The symmetric split backward with the allocations of ``ops.attention_alibi_backward``: dqkv and the workspace per call."""
    lib = _lib.load()
    b, _, t = qkv.shape
    dqkv = torch.empty_like(qkv)
    nbytes = int(lib.agx_attention_backward_workspace_bytes(b, H, t))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
    _lib.check(lib.agx_attention_alibi_backward_ex(ops._ptr(qkv), ops._ptr(slopes), ops._ptr(out), ops._ptr(dout), ops._ptr(dqkv),
                                                   ops._ptr(ws), nbytes, b, H, DH, t, float(DH ** 0.5), ops._stream()),
               "agx_attention_alibi_backward_ex")
    return dqkv


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    slopes = (2.0 ** (-8.0 / torch.arange(H, 0, -1))).to(dev)
    attn = dict(heads=H, head_dim=DH, scale_div=DH ** 0.5)
    cases = []          # (name, fn, calls per round, warm-up calls)

    def add(name, fn, calls, warm):
        cases.append((name, fn, calls, warm))

    for t in LENGTHS:
        qkv = (0.7 * torch.randn(B, 3 * H * DH, t, generator=gen)).to(dev)
        dout = torch.randn(B, H * DH, t, generator=gen).to(dev)
        out_s = ops.attention_alibi(qkv, slopes, **attn, flash=True)
        out_c = ops.attention_alibi_causal(qkv, None, slopes, **attn)
        fc, bc = (200, 50) if t <= 256 else (40, 8)
        sym_f = lambda qkv=qkv: ops.attention_alibi(qkv, slopes, **attn, flash=True)                       # noqa: E731
        sym_b = lambda qkv=qkv, out=out_s, dout=dout: split_backward(qkv, slopes, out, dout)                # noqa: E731
        add(f"symmetric fwd T={t}", sym_f, fc, 20)
        add(f"causal fwd T={t}", lambda qkv=qkv: ops.attention_alibi_causal(qkv, None, slopes, **attn), fc, 20)
        add(f"symmetric fwd T={t} again", sym_f, fc, 0)
        add(f"symmetric split bwd T={t}", sym_b, bc, 5)
        add(f"causal bwd T={t}", lambda qkv=qkv, out=out_c, dout=dout: ops.attention_alibi_causal_backward(qkv, slopes, out, dout, **attn),
            bc, 5)
        add(f"symmetric split bwd T={t} again", sym_b, bc, 0)
    t = LENGTHS[-1]
    q1 = (0.7 * torch.randn(B, H * DH, 1, generator=gen)).to(dev)
    cache = (0.7 * torch.randn(B, 2 * H * DH, t, generator=gen)).to(dev)
    add(f"causal cached step tq=1 tk={t}", lambda: ops.attention_alibi_causal(q1, cache, slopes, **attn, q_pos0=t - 1, tk=t), 200, 20)

    for _, fn, _, warm in cases:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in cases}
    for _ in range(ROUNDS):
        for name, fn, calls, _ in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(1e3 * start.elapsed_time(stop) / calls)
    print(f"# HIP-event times, us per call (wrapper included), B={B} H={H} Dh={DH}, fp32; {ROUNDS} rounds, cases alternated")
    print(f"# {'case':<40}{'calls':>7}{'median':>11}{'min':>11}{'max':>11}")
    for name, _, calls, _ in cases:
        ts = times[name]
        print(f"{name:<42}{calls:7d}{statistics.median(ts):11.1f}{min(ts):11.1f}{max(ts):11.1f}")


if __name__ == "__main__":
    main()
